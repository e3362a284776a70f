// qpd_fast_plan.hpp -- what the fast engine's host code (qpd_capi.hip) and its
// kernels (qpd_fast.hip, qpd_fast_pre.hpp) share: the launch's plan struct, the
// row access in LDS and the global slab, the table fetch.
#pragma once
#include "qpd_fast_switches.hpp"

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qpd_mop.hpp"

namespace qpd {

struct FastPlan {
    int32_t N, n, K, L, v, gs, fpw, nops, max_r1;
    int32_t in_vec;               // per launch: input rows are 16-byte aligned
    int32_t in_shift;             // per launch: log2 int32 words per frame row of `in` (n: channel
                                  // symbols; n - 2: pre-pass rows, root_pre_kernel)
    int32_t out_k;                // output bits per frame: K, or A (CRC-aided kinds)
    int32_t ca_A, crc_n;          // crc_n > 0: CRC-aided output (ca_winner)
    uint32_t crc_q;
    const uint32_t *info_mask;    // [N/32] information-position mask
    int32_t lds_rows, glb_rows, lds_from;
    int32_t R0_row, R0_lds;      // root partial sums (R[0])
    int32_t H_row, K_row, I_row;  // R1 scratch (global)
    const uint32_t *f_tab;        // [N-1][32] nibble-packed f tables
    const uint32_t *g_tab;        // [N-1][64] nibble-packed g tables (u=0: dwords 0..31)
    const double *vcl;            // [rows][N][v]
    const MOp *ops;
    const int32_t *info_pos;
    const uint16_t *r1_rank;      // FastSCL R1 (<= 32 elements): [temp][v] rank << 1 | sign, per node at op.tab
    uint32_t *scratch;            // [waves][glb_rows][64]
    int32_t *err;
    uint32_t *task_ctr;           // QPD_DYN task queue: tasks taken (never reset; see wave_take)
    uint32_t task_base;           // per launch: the counter's value when this launch's takes begin
    // Frozen-prefix stages (lut_prefix_kernel).  A stage writes, per frame f and path p,
    // its live rows (OP_EXPORT) and metric (two words from pm_off) as a record of pfx_rec
    // words in a buffer of its own, interleaved so that the 64 lanes of a wave store 64
    // consecutive words: word w of (f, p) at ((f >> G) * pfx_rec + w) * 64 + (f mod 2^G) *
    // 2^PS + p, pfx_geo = G | PS << 8 (2^G frames of 2^PS paths per 64 words; stage 1:
    // G = 6, PS = 0; stage 2: G = 4, PS = 2).  OP_IMPORT (MF_XBUF) reads records back with
    // the buffer address, record words, geometry and live paths in the op record (u_row |
    // r_row << 32, tab, vrow, tab2), not in the plan: plan fields the decode loop reads
    // cost it SGPRs (spill 149 -> 158).
    uint32_t *pfx;
    int32_t pfx_rec, pfx_geo, pm_off;
#ifdef QPD_STAMPS
    unsigned long long *stamps;   // diagnostic builds: [64] per-class cycle / count accumulators
#endif
};

// Decode status (qpd_decode_status), per launch: the decode kernels' last argument,
// read by the ST instantiations' tail alone.  Not part of FastPlan: the plan is the
// first kernel argument, and growing it moves the others -- this way the plain
// instantiations compile to the instructions they had before the status existed.
struct FastStatus {
    uint32_t crc_mask;   // XORed onto the CRC register's low bits before the compare (ca_winner)
    double *st_metric;   // [B] path metric of the output path, or NULL
    uint8_t *st_pass;    // [B] 1 = the output path passed the CRC, or NULL
    // List output (qpd_decode_list), read by the LIST instantiations' tail alone: the
    // candidates from the launch's first frame on, in argsort(PML) order.  After the
    // status fields: the last argument's tail, so that no other offset moves.
    uint8_t *ls_bits;    // [B][L][K] every path's decisions at the information positions
    double *ls_metric;   // [B][L] or NULL
    uint8_t *ls_pass;    // [B][L] or NULL: the path's own CRC compare
    int32_t *ls_chosen;  // [B] or NULL: the candidate whose bits `out` receives
    // Mask search (qpd_decode_search), read by the LIST instantiations' tail alone, again at
    // the end.  sr_set != NULL: a search call -- ls_bits is NULL (no candidate bits are
    // gathered), ls_metric / ls_chosen are the call's cand_metric / hit_rank, st_metric its
    // metric, and the output path is chosen by the set compare (ca_winner_ranked).
    const uint32_t *sr_set;  // [sr_n] the masks' register values >> (crc_n - chk), in a buffer of the decoder's
    int32_t sr_n;
    uint32_t *sr_syndrome;   // [B][L] or NULL: every path's CRC syndrome at its rank
    int32_t *sr_hit;         // [B] or NULL: the lowest mask index that passes the output path, -1: none
};

// Row access in either space.  `in_lds` is wave-uniform.  The global slab is
// reached through a buffer descriptor (32-bit lane offsets; distinct
// instructions, so the compiler never folds the two spaces into one flat
// access that would wait on both counters).
// A wave's `ns` frame sets interleave their rows, in LDS and in the slab: row r
// of set s is the wave's row r * ns + s.  The sets share one LDS base and one
// slab descriptor and a set's view differs only by s rows -- an immediate
// offset in its LDS / buffer instructions (`so` bytes, constant after the set
// loops unroll) instead of a base register and a descriptor per set.
struct Mem {
    uint32_t *lds;              // this set's LDS row 0 (the wave's base + s rows)
    uint32_t *gp;               // this set's slab row 0 (R1 argsort arrays)
    __amdgpu_buffer_rsrc_t rs;  // the wave's slab, all sets
    int so;                     // this set's byte offset in a slab row group (s * 256)
    int ns;                     // frame sets of the wave: the row stride in rows
    __device__ __forceinline__ int rw(int row) const { return row * ns * 64; }  // words to row `row`
    // the view of set s (runtime) from set 0's
    __device__ __forceinline__ Mem set(int s) const {
        Mem m = *this;
        m.lds = lds + s * 64;
        m.gp = gp + s * 64;
        m.so = so + s * 256;
        return m;
    }
    // `row` wave-uniform: it rides in the buffer op's SGPR offset
    __device__ __forceinline__ uint32_t ld(bool in_lds, int row, int lane) const {
        if (in_lds) return lds[rw(row) + lane];
        return __builtin_amdgcn_raw_buffer_load_b32(rs, lane * 4, row * ns * 256 + so, QPD_SLAB_AUX);
    }
    __device__ __forceinline__ void st(bool in_lds, int row, int lane, uint32_t v) const {
        if (in_lds)
            lds[rw(row) + lane] = v;
        else
            __builtin_amdgcn_raw_buffer_store_b32(v, rs, lane * 4, row * ns * 256 + so, QPD_SLAB_AUX);
    }
    // any row (per-lane)
    __device__ __forceinline__ uint32_t ldv(bool in_lds, int row, int lane) const {
        if (in_lds) return lds[rw(row) + lane];
        return __builtin_amdgcn_raw_buffer_load_b32(rs, (rw(row) + lane) * 4 + so, 0, QPD_SLAB_AUX);
    }
    __device__ __forceinline__ void stv(bool in_lds, int row, int lane, uint32_t v) const {
        if (in_lds)
            lds[rw(row) + lane] = v;
        else
            __builtin_amdgcn_raw_buffer_store_b32(v, rs, (rw(row) + lane) * 4 + so, 0, QPD_SLAB_AUX);
    }
};

// Table dword `at + ldw` (at wave-uniform, ldw = the lane's dword) through a
// buffer descriptor: the uniform part rides in the SGPR offset, so a table
// fetch costs no per-lane 64-bit address arithmetic.
__device__ __forceinline__ uint32_t tab_ld(const uint32_t *base, int at, int ldw) {
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, 0x7fffffff, 0x00020000);
    return __builtin_amdgcn_raw_buffer_load_b32(r, ldw * 4, at * 4, 0);
}

}  // namespace qpd
