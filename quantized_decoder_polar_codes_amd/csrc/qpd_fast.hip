// qpd_fast.hip -- the fast gfx950 LUT decode kernel (one table per node, v <= 16).
//
// Same algorithm, traversal and list management as the generic kernel
// (qpd_generic.hip: one lane per list path, G = pow2 >= L lanes per frame,
// per-depth 4-bit slot pointers instead of deep copies), laid out for the
// CDNA4 memory hierarchy and for instruction count:
//
//  * Host-compiled micro-op records (MOp, 64 B, one s_load_dwordx16 each)
//    carry every row offset, shift and flag an op needs, so the wave-uniform
//    interpreter does almost no scalar arithmetic per op.
//  * Symbols are 4-bit nibbles, 8 per dword.  Per tree depth d a path owns
//    S[d] (symbols of the active depth-d node), U[d] (partial sums of the
//    finished left child) and R[d] (partial sums of a finished right child).
//    Deep levels (d >= lds_from) sit in LDS, shallow levels in a per-wave
//    global slab; both are laid out [row][64 lanes].  LDS instructions of one
//    wave complete in order, so LDS-only ops need no barrier.
//  * The last three tree levels of every plain subtree are one BOT3 op held
//    entirely in registers: 8 symbols in, 8 leaves decided (with list forks
//    moving the whole in-register state from the parent lane), 8 partial-sum
//    bits out -- 21 interpreted ops become one straight-line block.
//  * The current node's f/g table sits in ONE VGPR per lane (f: 256 nibbles =
//    32 dwords, g: 512 nibbles = 64 dwords), read with ds_bpermute; the next
//    op's table / leaf quanta row are prefetched while the current op runs.
#pragma once
#include "qpd_fast_switches.hpp"

#include "qpd_fast_plan.hpp"
#include "qpd_fast_lookup.hpp"
#include "qpd_fast_select.hpp"
#include "qpd_fast_bot.hpp"
#include "qpd_fast_special.hpp"

// The tail's mode (lut_fast_kernel's ST): the bits alone, + the decode status
// (qpd_decode_status), + the whole list (qpd_decode_list).
#define QPD_TAIL_PLAIN 0
#define QPD_TAIL_ST 1
#define QPD_TAIL_LIST 2

// A unit compiled with QPD_STATUS_UNIT (the *_st.hip wrappers) instantiates the ST
// kernels and names its lookup function <name>_st; with QPD_LIST_UNIT (the *_ls.hip
// wrappers) the LIST kernels, <name>_ls.
#if defined(QPD_LIST_UNIT)
#define QPD_ST QPD_TAIL_LIST
#define QPD_UNIT_FN(f) f##_ls
#elif defined(QPD_STATUS_UNIT)
#define QPD_ST QPD_TAIL_ST
#define QPD_UNIT_FN(f) f##_st
#else
#define QPD_ST QPD_TAIL_PLAIN
#define QPD_UNIT_FN(f) f
#endif

namespace qpd {

// NS frame sets per wave (see qpd_fast_select.hpp); L8: list decoders with L = 8; W16: SCL-LUT and
// FastSCL-LUT with 9 <= L <= 16 (lane groups of 16, select_survivors16; FastSCL-LUT's
// special nodes through the single-set special_op, R1 nodes with up to 15 layers).
// LDS: NS * (lds_rows + 2) rows, set-interleaved (see Mem): a set's rows
// 0..lds_rows-1 (grouped by depth, see FastLayout), then its selection scratch
// as rows lds_rows (64 slots) and lds_rows + 1 (junk slots).
// Global slab: NS * glb_rows rows per workgroup, set-interleaved.
// PFX: the frozen-prefix kernel (lut_prefix_kernel below; one set, gs = 1, no
// tail, `out` unused).  A template argument rather than a wrapper around a
// shared body: the wrapper moved the decode kernels' register allocation
// (FastSCL-LUT 63 -> 71 ms per 2^21 frames, profiles/r03ac_ab.txt).
//
// `ops` is its own __restrict__ argument (= P.ops) so that the compiler can
// prove the op records are never written and fetch them with scalar loads
// instead of vector loads + readfirstlane, which drain vmcnt at every op.
// PW1: one pointer word per path (PathT; the host packed the op list's fields).
// ST: the tail also writes the decode status (qpd_decode_status: the output path's
// metric and CRC verdict, the CRC mask) -- instantiations of their own (the *_st.hip
// units), so that the plain decode kernels compile to what they are without it.
// ST = QPD_TAIL_LIST (the *_ls.hip units): the tail writes every path of the list
// instead (qpd_decode_list, the LIST block below).
template <int KIND, int NS, bool L8, bool R1L = false, bool PFX = false, bool PW1 = false, bool W16 = false,
          int ST = QPD_TAIL_PLAIN>
__global__ __launch_bounds__(64, NS == 3 ? QPD_WPE3
                                : W16 ? QPD_WPE_W16
                                : NS == 2 ? (KIND == K_SCL_LUT && !PFX ? QPD_WPE2_SCL : KIND == K_FASTSCL_LUT ? QPD_WPE2_FSCL : QPD_WPE2)
                                : KIND == K_FASTSCL_LUT ? QPD_WPE_FSCL : QPD_WPE1) void lut_fast_kernel(FastPlan P, const int32_t *__restrict__ in, int64_t B,
                                                               uint8_t *__restrict__ out,
                                                               const MOp *__restrict__ ops, FastStatus SO) {
    constexpr bool kList = (KIND == K_SCL_LUT || KIND == K_FASTSCL_LUT);
    static_assert(!W16 || (!L8 && (KIND == K_SCL_LUT || (KIND == K_FASTSCL_LUT && !R1L && !PFX))),
                  "W16: SCL-LUT / FastSCL-LUT list sizes 9..16");
    static_assert(!ST || (kList && !PFX), "ST: the list kinds' decode kernels");
    constexpr int LM = L8 ? 8 : W16 ? 16 : 0;  // list mode of the leaf forks (leaf_fork)
    // staged BOT3 loads: the list kinds (SCL-LUT, FastSCL-LUT)
    constexpr bool kLazy = QPD_BOT3_LAZY && kList;
    constexpr bool kFast = (KIND == K_FASTSC_LUT || KIND == K_FASTSCL_LUT) && !(QPD_EXP_FSCL & 256);
    // channel reads inside the decode (MF_CHAN: codes without the root pre-pass); the
    // one-pointer-word SCL-LUT instantiations run only op lists with the pre-pass
    // (plan_fast; +1.1 % SCL-LUT, -1.3 % when FastSCL-LUT's dropped them too, r05z5)
    constexpr bool kChan = !(PW1 && KIND == K_SCL_LUT);
    // rows in lookup order (QPD_ROW_BYTEIDX, qpd_fast_switches.hpp): the plain kinds; plan_fast
    // marks their ops MF_LO by the same rule (FastHostPlan::row_lo)
    constexpr bool kLO = QPD_ROW_BYTEIDX != 0 && (KIND == K_SC_LUT || KIND == K_SCL_LUT);
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_dyn[];
    // list kinds at two frame sets: the f / g ops' byte tables (stage_tab) and the
    // folded descents (MF_FF), 768 B at the start of the wave's LDS -- a constant
    // address, so that every byte-table lookup is a ds_read_u8 of its index with the
    // table's place in the instruction's offset field (one VALU add per lookup less
    // than from a base in a register); then the rows of all sets, interleaved, and
    // each set's selection scratch as its next two rows (set s's slots at sel_all +
    // s * 64, its junk slots NS * 64 words on)
    constexpr bool kLdsTab = kList && NS >= 2 && !QPD_EXP_NO_LDSTAB;
    constexpr int kTabWords = kLdsTab ? 192 : 0;  // (qpd_capi.hip: lds_tab_bytes)
    uint8_t *const tb = (uint8_t *)lds_dyn;
    uint32_t *const lds_rows = lds_dyn + kTabWords;
    const int sstride = 64;
    int *const sel_all = (int *)(lds_rows + NS * P.lds_rows * 64);
    Mem Mv[NS];
    {
        uint32_t *const slab = P.scratch + (size_t)blockIdx.x * NS * P.glb_rows * 64;
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc(slab, 0, NS * P.glb_rows * 256 * QPD_EXP_SLABMUL, 0x00020000);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            Mv[s].lds = lds_rows + s * 64;
            Mv[s].gp = slab + s * 64;
            Mv[s].rs = rs;
            Mv[s].so = s * 256;
            Mv[s].ns = NS;
        }
    }
    const int gs = P.gs;
    const int L = kList ? P.L : 1;
    const int N = P.N;
    const int64_t fpw = P.fpw;  // frames per set
    const int64_t ntasks = (B + NS * fpw - 1) / (NS * fpw);
    const double kInf = __builtin_huge_val();

    // Tasks: the first blockIdx.x, then (QPD_DYN) the next untaken one from
    // the queue -- every SIMD stays busy to the end whatever the residency --
    // or the grid-stride successor.
    for (int64_t task = blockIdx.x; task < ntasks;
         task = QPD_DYN ? (int64_t)gridDim.x + wave_take(P.task_ctr, P.task_base) : task + gridDim.x) {
#ifdef QPD_POISON
        // Diagnosis builds only: every LDS word and slab row of this wave set to
        // QPD_POISON at the start of each task, so that a read of a row no op of
        // this task wrote shows up as a parity difference.
        for (int i = threadIdx.x; i < NS * (P.lds_rows * 64 + kSelInts); i += 64) lds_rows[i] = (uint32_t)QPD_POISON;
        for (int r = 0; r < NS * P.glb_rows; ++r) Mv[0].gp[r * 64 + threadIdx.x] = (uint32_t)QPD_POISON;
        wave_sync();
#endif
        PathT<PW1> stv[NS];
        {
            const int lane = threadIdx.x, gl = lane & (gs - 1);
            uint64_t self = 0;
            for (int d = 0; d < kMaxDepth; ++d) self |= (uint64_t)gl << (4 * d);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                stv[s].pm = (gl == 0) ? 0.0 : kInf;
                stv[s].ps = self;
                stv[s].U() = self;  // (PW1: the same word)
            }
        }
#ifdef QPD_STAMPS
        uint64_t stamp_acc = 0, stamp_cnt = 0;
#endif
        MOp nxt = ops[0];
        Pre pre = fetch_pre(P, nxt, threadIdx.x, threadIdx.x < P.v ? threadIdx.x : 0);
        for (int oi = 0; oi < P.nops; ++oi) {
            // Re-derive the lane constants every op: without this the compiler
            // hoists dozens of lane-derived addresses out of the op loop and
            // pins them in VGPRs for the whole kernel (spills, low occupancy).
            int lane = threadIdx.x;
            asm volatile("" : "+v"(lane));
            const int gl = lane & (gs - 1);
            const int gbase = lane & ~(gs - 1);
            const int vlane = lane < P.v ? lane : 0;
            const int32_t *yv[NS];  // frame rows of `in` (read by MF_CHAN / MF_PRE ops only)
            const int gsh = __builtin_ctz(gs);
            if (nxt.flags & (MF_CHAN | MF_PRE)) {  // wave-uniform: no per-lane address math on other ops
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    int64_t f = (task * NS + s) * fpw + (lane >> gsh);
                    if (f >= B) f = B - 1;
                    yv[s] = in + (f << P.in_shift);
                }
            } else {
#pragma unroll
                for (int s = 0; s < NS; ++s) yv[s] = in;
            }
            if (nxt.flags & MF_SYNC) wave_sync();  // before the next prefetch is issued
            const MOp op = nxt;
            const Pre cur = pre;
#ifdef QPD_STAMPS
            __builtin_amdgcn_s_waitcnt(0);
            const uint64_t stamp_t0 = __builtin_amdgcn_s_memtime();
#endif
            // the next op's operands; a BOT3 issues them itself, late (see bot3_op)
            if (oi + 1 < P.nops) {
                nxt = ops[oi + 1];
                if (!kLazy || op.type != OP_BOT3) pre = fetch_pre(P, nxt, lane, vlane);
            }
            const int fl = op.flags;
            // special nodes, FastSCLUT.cpp:46-107 / FastSCLLUTDecoder.cpp:82-213
            auto run_special = [&]() {
              if constexpr (kFast) {
                  // the sets one after the other, one copy of the code: set s runs in
                  // stv[0] (the sets' states rotate; back in place after NS steps) --
                  // the special nodes' code is not in the instruction cache twice
                  if constexpr (KIND == K_FASTSCL_LUT && L8) {
                    if ((op.type == OP_R0 || op.type == OP_REP) && !(QPD_EXP_FSCL & 512)) {
                        r0rep_multi<kLdsTab, R1L>(P, Mv, op, stv, sel_all, sstride, gl, gbase, lane, cur.T2, tb);
                        return;
                    }
                    if (op.type == OP_R1 && (op.cnt <= stl::kThreshold || (fl & MF_R1_LDS)) && !(QPD_EXP_FSCL & 1024)) {
                        r1_multi<kLdsTab, R1L>(P, Mv, op, stv, sel_all, sstride, gl, gbase, lane, lds_rows, cur.T2, tb);
                        return;
                    }
                    // without R1L every R1 node of > 16 elements has its LDS tail (the host
                    // takes the R1L instantiation otherwise) and FastSCL-LUT has no SPC ops
                    // (H7): nothing is left for the generic special_op
                    if constexpr (!R1L) return;
                  }
#if QPD_SPEC_ROT
#pragma unroll 1
                  for (int s = 0; s < NS; ++s) {
                    special_op<kList, LM, R1L>(P, Mv[0].set(s), op, stv[0], sel_all + sstride * s, NS * sstride, gl, gbase,
                                               L, lane, lds_rows);
                    rotate_sets(stv);
                  }
#else
#pragma unroll
                  for (int s = 0; s < NS; ++s)
                    special_op<kList, LM, R1L>(P, Mv[s], op, stv[s], sel_all + sstride * s, NS * sstride, gl, gbase, L, lane,
                                               lds_rows);
#endif
              }
            };
            switch (op.type) {
                case OP_BOT3:
                    if constexpr (KIND == K_FASTSCL_LUT && L8 && !QPD_EXP_NO_BOTX) {
                        if (fl & MF_BOTX) {
                            if (kLazy && oi + 1 < P.nops) pre = fetch_pre(P, nxt, lane, vlane);
                            botx_op<kLdsTab, kChan>(P, Mv, op, yv, stv, cur.T, cur.T2, gl, gbase, L, sel_all, sstride, lane, tb);
                            break;
                        }
                    }
                    bot3_op<kList, LM, kLazy, kLdsTab, kChan, kLO>(P, Mv, op, yv, stv, cur.T, cur.T2, gl, gbase, L, sel_all, sstride, lane, [&]() {
                        if (oi + 1 < P.nops) pre = fetch_pre(P, nxt, lane, vlane);
                    }, tb);
                    break;
                case OP_F:
                case OP_G: {
                    int src[NS], usrc[NS];
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        src[s] = gbase + pfield(stv[s].ps, op.sh_src);
                        usrc[s] = gbase + pfield(stv[s].U(), op.sh_u);
                    }
                    if constexpr (kLdsTab) {
                        if (fl & MF_FF) {  // + the left child's f (fuse_descent)
                            const int key = ((fl & MF_DST_LDS) ? 1 : 0) | ((fl & MF_FF_DL) ? 2 : 0);
                            stage_tab(tb, cur.T, op.type == OP_F ? (lane & 31) : gtab_dw(lane));
                            stage_tab(tb + 512, cur.T2, lane & 31);
#define QPD_FF(G, D_, C_) ff_op<G, D_, C_, NS, kLO>(Mv, op, src, usrc, tb, lane)
                            if (op.type == OP_F) {
                                if (key == 0) QPD_FF(false, 0, 0);
                                else if (key == 2) QPD_FF(false, 0, 1);
                                else QPD_FF(false, 1, 1);
                            } else {
                                if (key == 0) QPD_FF(true, 0, 0);
                                else if (key == 2) QPD_FF(true, 0, 1);
                                else QPD_FF(true, 1, 1);
                            }
#undef QPD_FF
#pragma unroll
                            for (int s = 0; s < NS; ++s) stv[s].ps = pset(pset(stv[s].ps, op.sh_dst, gl), op.pad1, gl);
                            break;
                        }
                    }
                    if (fl & MF_GSEL)
                        gsel_op<NS, kLO>(Mv, op, yv, usrc, lane);
                    else if (NS >= 2 && !(fl & (MF_CHAN | MF_PRE))) {  // (one-set FastSCL: smaller code measured faster)
                        // row spaces of source and destination fixed per instantiation
                        const int key = ((fl & MF_SRC_LDS) ? 1 : 0) | ((fl & MF_DST_LDS) ? 2 : 0);
                        if constexpr (kLdsTab)
                            if (op.cnt >= 8) stage_tab(tb, cur.T, op.type == OP_F ? (lane & 31) : gtab_dw(lane));
#define QPD_FG(G, S_, D_) fg_op<G, true, NS, S_, D_, kLdsTab, kLO>(P, Mv, op, yv, src, usrc, cur.T, lane, tb)
                        // (S[d] in LDS puts S[d + 1] in LDS too: no key 1 variant)
                        if (op.type == OP_F) {
                            if (key == 0) QPD_FG(false, 0, 0);
                            else if (key == 2) QPD_FG(false, 0, 1);
                            else QPD_FG(false, 1, 1);
                        } else {
                            if (key == 0) QPD_FG(true, 0, 0);
                            else if (key == 2) QPD_FG(true, 0, 1);
                            else QPD_FG(true, 1, 1);
                        }
#undef QPD_FG
                    } else if (kChan && (fl & MF_CHAN)) {
                        if (op.type == OP_F) fg_chan_op<false, NS, kLO>(P, Mv, op, yv, usrc, cur.T, lane);
                        else fg_chan_op<true, NS, kLO>(P, Mv, op, yv, usrc, cur.T, lane);
                    } else if (op.type == OP_F)
                        fg_op<false, false, NS, -1, -1, false, kLO>(P, Mv, op, yv, src, usrc, cur.T, lane);
                    else
                        fg_op<true, false, NS, -1, -1, false, kLO>(P, Mv, op, yv, src, usrc, cur.T, lane);
#pragma unroll
                    for (int s = 0; s < NS; ++s) stv[s].ps = pset(stv[s].ps, op.sh_dst, gl);
                    break;
                }
                case OP_LEAF_L:
                case OP_LEAF_R: {
                    const bool right = op.type == OP_LEAF_R;
                    const bool frozen = op.cnt != 0;
                    double dm[NS];
                    uint32_t none[NS][1], dec[NS];
                    bool moved[NS];
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        dm[s] = 0;
                        none[s][0] = 0;
                        if (kList || !frozen) {
                            const uint32_t W = sym_word<kChan>(P, Mv[s], op, yv[s], gbase + pfield(stv[s].ps, op.sh_src), 0, 2);
                            uint32_t idx = QPD_LEAF_T ? (W & 0xFFu) : (((W & 15u) << 4) | ((W >> 4) & 15u));  // (leaf_idx)
                            if (right)
                                idx |= (Mv[s].ld(fl & MF_U_LDS, op.u_row, gbase + pfield(stv[s].U(), op.sh_u)) & 1u) << 8;
                            dm[s] = shfld(cur.V, (int)lut4(cur.T, idx));  // vcl[n-1][k][s] (H3)
                        }
                    }
                    leaf_decide<kList, LM>(stv, dm, frozen, gl, gbase, L, lane, sel_all, sstride, none, dec, moved);
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        Mv[s].st(fl & MF_DST_LDS, op.dst_row, lane, dec[s]);
                        if (!right) stv[s].U() = pset(stv[s].U(), op.sh_dst, gl);
                    }
                    break;
                }
                case OP_COMB: {
                    const int ctemp = op.cnt;
                    const bool ul = fl & MF_U_LDS, rl = fl & MF_R_LDS, dl = fl & MF_DST_LDS;
                    if (ctemp < 32) {
                        const uint32_t m = (1u << ctemp) - 1u;
                        uint32_t u[NS], r[NS];
#pragma unroll
                        for (int s = 0; s < NS; ++s) {
                            u[s] = Mv[s].ld(ul, op.u_row, gbase + pfield(stv[s].U(), op.sh_u)) & m;
                            r[s] = Mv[s].ld(rl, op.r_row, lane) & m;
                        }
#pragma unroll
                        for (int s = 0; s < NS; ++s) Mv[s].st(dl, op.dst_row, lane, (u[s] ^ r[s]) | (r[s] << ctemp));
                    } else {
                        const int cw = ctemp >> 5;  // 1, 2 or a multiple of 4
                        int usrc[NS];
#pragma unroll
                        for (int s = 0; s < NS; ++s) usrc[s] = gbase + pfield(stv[s].U(), op.sh_u);
                        // 4 words of every set per round: all their loads in flight together
                        for (int w0 = 0; w0 < cw; w0 += 4) {
                            uint32_t u[NS][4], r[NS][4];
#pragma unroll
                            for (int s = 0; s < NS; ++s)
#pragma unroll
                                for (int k = 0; k < 4; ++k) {
                                    u[s][k] = r[s][k] = 0u;
                                    if (k == 0 || w0 + k < cw) {
                                        u[s][k] = Mv[s].ld(ul, op.u_row + w0 + k, usrc[s]);
                                        r[s][k] = Mv[s].ld(rl, op.r_row + w0 + k, lane);
                                    }
                                }
#pragma unroll
                            for (int s = 0; s < NS; ++s)
#pragma unroll
                                for (int k = 0; k < 4; ++k)
                                    if (k == 0 || w0 + k < cw) {
                                        Mv[s].st(dl, op.dst_row + w0 + k, lane, u[s][k] ^ r[s][k]);
                                        Mv[s].st(dl, op.dst_row + cw + w0 + k, lane, r[s][k]);
                                    }
                        }
                    }
                    if (!(fl & MF_TO_R)) {
#pragma unroll
                        for (int s = 0; s < NS; ++s) stv[s].U() = pset(stv[s].U(), op.sh_dst, gl);
                    }
                    break;
                }
                case OP_IMPORT:
                    if constexpr (KIND == K_SCL_LUT) {  // a frozen-prefix stage's records (lut_prefix_kernel)
                        const int live = op.tab2;
#pragma unroll
                        for (int s = 0; s < NS; ++s) {
                            const bool dl = fl & MF_DST_LDS;
                            if (fl & MF_ZERO) {  // the prefix's partial sums: frozen zeros
                                for (int w = 0; w < op.cnt; ++w) Mv[s].st(dl, op.dst_row + w, lane, 0u);
                                continue;
                            }
                            int64_t f = (task * NS + s) * fpw + (lane >> gsh);
                            if (f >= B) f = B - 1;
                            const int G = op.vrow & 255;
                            // the record of this lane's path (dead paths: path 0's)
                            const uint32_t *src = (const uint32_t *)(((uint64_t)(uint32_t)op.r_row << 32) | (uint32_t)op.u_row) +
                                                  (((f >> G) * op.tab) << 6) + ((f & ((1 << G) - 1)) << (op.vrow >> 8)) +
                                                  (gl < live ? gl : 0);
                            if (fl & MF_PM) {
                                const uint64_t b = (uint64_t)src[op.src_row << 6] | ((uint64_t)src[(op.src_row + 1) << 6] << 32);
                                stv[s].pm = gl < live ? __builtin_bit_cast(double, b) : kInf;
                                            } else {  // live rows into every path's own column
                                for (int w = 0; w < op.cnt; ++w) Mv[s].st(dl, op.dst_row + w, lane, src[(op.src_row + w) << 6]);
                            }
                        }
                    }
                    break;
                case OP_EXPORT:
                    if constexpr (KIND == K_SCL_LUT && PFX) {  // the row of this path's lineage
#pragma unroll
                        for (int s = 0; s < NS; ++s) {
                            const int64_t f = (task * NS + s) * fpw + (lane >> gsh);
                            const int at = (fl & MF_VIA_PS)   ? gbase + pfield(stv[s].ps, op.sh_src)
                                           : (fl & MF_VIA_PU) ? gbase + pfield(stv[s].U(), op.sh_src)
                                                              : lane;
                            const int G = P.pfx_geo & 255;
                            uint32_t *dst = P.pfx + (((f >> G) * P.pfx_rec) << 6) + ((f & ((1 << G) - 1)) << (P.pfx_geo >> 8)) + gl;
                            for (int w = 0; w < op.cnt; ++w) {
                                const uint32_t x = Mv[s].ld(fl & MF_SRC_LDS, op.src_row + w, at);
                                if (f < B) dst[(op.dst_row + w) << 6] = x;
                            }
                        }
                    }
                    break;
                default:
                    if constexpr (kFast) run_special();
                    break;
            }
#ifdef QPD_STAMPS
            __builtin_amdgcn_s_waitcnt(0);
            {
                const uint64_t dt = __builtin_amdgcn_s_memtime() - stamp_t0;
#ifdef QPD_STAMPS_DEPTH  // F / G / COMB by depth: 0-7 / 8-15 / 16-23; BOT3 24; leaves 25; specials 26-29
                const int dd = op.d < 7 ? op.d : 7;
                const int cls = op.type == OP_F ? dd : op.type == OP_G ? 8 + dd : op.type == OP_COMB ? 16 + dd
                              : op.type == OP_BOT3 ? ((fl & MF_BOTX) ? 30 : 24) : (op.type == OP_LEAF_L || op.type == OP_LEAF_R) ? 25
                              : 26 + (op.type - OP_R0) % 4;
#else
                const int cls = op.type == OP_R1 ? 24 + (op.cnt > 16) + (op.cnt > 8) : 2 * op.type + ((fl & MF_SYNC) ? 1 : 0);
#endif
                if ((int)(threadIdx.x & 31) == cls) stamp_acc += dt;
                if ((int)(threadIdx.x & 31) == cls) stamp_cnt += 1;
            }
#endif
        }
        if constexpr (PFX) {  // the stage's path metrics next to its rows; no decisions to output
            const int gl = threadIdx.x & (gs - 1);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const int64_t f = (task * NS + s) * fpw + (threadIdx.x >> __builtin_ctz(gs));
                const int G = P.pfx_geo & 255;
                uint32_t *dst = P.pfx + (((f >> G) * P.pfx_rec) << 6) + ((f & ((1 << G) - 1)) << (P.pfx_geo >> 8)) + gl;
                const uint64_t b = __builtin_bit_cast(uint64_t, stv[s].pm);
                if (f < B) {
                    dst[P.pm_off << 6] = (uint32_t)b;
                    dst[(P.pm_off + 1) << 6] = (uint32_t)(b >> 32);
                }
            }
            wave_sync();  // the rows are reused by the next task, as after the tail below
            continue;
        }
#ifdef QPD_STAMPS
        __builtin_amdgcn_s_waitcnt(0);
        const uint64_t stamp_t2 = __builtin_amdgcn_s_memtime();
#endif

        // Root partial sums -> u = x F^{(x)n} (FastSCLUT.cpp:186-198), R[0] rows;
        // output u[info] of the winning path (SCLLUTDecoder.cpp:244-252).
        // FastSCL-LUT: the lane constants re-derived here too -- otherwise the compiler
        // computes the tail's lane-dependent addresses once before the task loop and
        // keeps them across the whole op loop in scratch (140 -> 80 B per lane, speed
        // unchanged).  Not for SCL-LUT: there the same change raised the SGPR spills
        // 148 -> 210 and cost 1.1 % (profiles/r06d_ab.txt); its scratch (112 B) is
        // written once before the task loop and read once per task, in the tail.
        int lane = threadIdx.x;
        if constexpr (KIND == K_FASTSCL_LUT) asm volatile("" : "+v"(lane));
        const int gl = lane & (gs - 1);
        const int gbase = lane & ~(gs - 1);
        const bool rl = P.R0_lds;
        const int r0 = P.R0_row;
        const int nwr = (N + 31) >> 5;
        const bool dword_out = (P.out_k & 3) == 0 && ((uintptr_t)out & 3) == 0;
        // Split tail (list decoders without CRC): the winner follows from the
        // path metrics alone, so only its root row is re-encoded, spread over
        // the frame's gs lanes (wpl words each; the cross-lane butterfly stages
        // by shuffles) and staged in this set's LDS rows for the output gather.
        const int wpl = nwr / gs;
        constexpr bool LS = ST == QPD_TAIL_LIST;  // every path's row is output: no split
        const bool split = !LS && kList && P.crc_n == 0 && nwr >= gs && wpl <= 8 && wpl <= P.lds_rows;
        if (!split) {  // every path re-encodes its own row (CRC-aided: each path's CRC is checked)
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const Mem &M = Mv[s];
                for (int w = 0; w < nwr; ++w) {
                    uint32_t x = M.ld(rl, r0 + w, lane);
                    if (N < 32) x &= (1u << N) - 1u;
                    M.st(rl, r0 + w, lane, polar_word(x));
                }
                for (int mw = 1; mw < nwr; mw *= 2)
                    for (int i = 0; i < nwr; i += 2 * mw)
                        for (int j = 0; j < mw; ++j)
                            M.st(rl, r0 + i + j, lane, M.ld(rl, r0 + i + j, lane) ^ M.ld(rl, r0 + i + mw + j, lane));
            }
            wave_sync();
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const Mem &M = Mv[s];
            if constexpr (LS) {
                // The list (qpd_decode_list): lane gl is list slot gl, its rank the path's
                // position in argsort(PML) (stable, L <= 16); candidate r = the lane of rank
                // r, whose K decisions the frame's gs lanes gather together (the output
                // gather below with that lane as its source), r = 0 .. L-1.  Each lane
                // writes its own metric and CRC verdict at its rank.
                const int rank = stable_rank(stv[s].pm, gl, gbase, L);
                bool passed = false, own = false;
                int best = 0, hit = -1;
                uint32_t syn = 0;
                // a mask search (qpd_decode_search; wave-uniform): the winner by the set compare
                // on each lane's syndrome, no candidate bits
                const bool search = SO.sr_set != nullptr;
                if (P.crc_n > 0)
                    best = ca_winner_ranked<true>(rank, gl, gbase, L, N, P.info_mask, P.ca_A, P.K - P.ca_A, P.crc_n, P.crc_q,
                                            [&](int w) { return M.ld(rl, r0 + w, lane); }, SO.crc_mask, &passed, &own,
                                            &syn, SO.sr_set, SO.sr_n, &hit);
                const int64_t frame = (task * NS + s) * fpw + lane / gs;
                const bool live = frame < B;
                auto bit = [&](int pos, int src) { return (M.ldv(rl, r0 + (pos >> 5), src) >> (pos & 31)) & 1u; };
                // nb decisions of the path in lane src -> dst, by the frame's lanes
                auto gather = [&](uint8_t *dst, int nb, int src, bool dw) {
                    if (dw) {  // four bytes per store; 4 stores' loads issued together
                        uint32_t *o32 = (uint32_t *)dst;
                        const int nc = nb >> 2;
                        for (int c0 = gl; c0 < nc; c0 += 4 * gs) {
                            uint32_t wv[4];
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                const int c = c0 + k * gs;
                                wv[k] = 0;
                                if (c < nc) {
                                    const int4 pp = *(const int4 *)(P.info_pos + 4 * c);
                                    wv[k] = bit(pp.x, src) | (bit(pp.y, src) << 8) | (bit(pp.z, src) << 16) |
                                            (bit(pp.w, src) << 24);
                                }
                            }
#pragma unroll
                            for (int k = 0; k < 4; ++k)
                                if (c0 + k * gs < nc) o32[c0 + k * gs] = wv[k];
                        }
                    } else {
                        for (int t = gl; t < nb; t += gs) dst[t] = (uint8_t)bit(P.info_pos[t], src);
                    }
                };
                const bool dword_ls = (P.K & 3) == 0 && ((uintptr_t)SO.ls_bits & 3) == 0;
                for (int r = 0; r < L && !search; ++r) {
                    // the group's lane of rank r (one per group; the ballot by the whole wave)
                    const uint64_t m = __ballot(gl < L && rank == r) >> gbase;
                    const int src = gbase + (__builtin_ctzll(m | (1ull << 63)) & (gs - 1));
                    if (r == 0 && P.crc_n == 0) best = src - gbase;  // the first minimum (H6)
                    if (live) gather(SO.ls_bits + (frame * L + r) * (int64_t)P.K, P.K, src, dword_ls);
                }
                const int crank = lane_read(rank, gbase + best);
                if (search) {  // the output path's hit and own metric, by the group's first lane
                    const int whit = lane_read(hit, gbase + best);
                    const double wpm = shfld(stv[s].pm, gbase + best);
                    if (live && gl < L && SO.sr_syndrome) SO.sr_syndrome[frame * L + rank] = syn;
                    if (live && gl == 0) {
                        if (SO.sr_hit) SO.sr_hit[frame] = whit;
                        if (SO.st_metric) SO.st_metric[frame] = wpm;
                    }
                }
                if (live) {
                    if (gl < L) {
                        if (SO.ls_metric) SO.ls_metric[frame * L + rank] = stv[s].pm;
                        if (SO.ls_pass) SO.ls_pass[frame * L + rank] = (uint8_t)own;
                    }
                    if (gl == 0 && SO.ls_chosen) SO.ls_chosen[frame] = crank;
                    if (out) gather(out + frame * P.out_k, P.out_k, gbase + best, dword_out);
                }
                continue;
            }
            int best = 0;
            bool passed = false;
            if (kList && P.crc_n > 0) {
                best = ca_winner(stv[s].pm, gl, gbase, L, N, P.info_mask, P.ca_A, P.K - P.ca_A, P.crc_n, P.crc_q,
                                 [&](int w) { return M.ld(rl, r0 + w, lane); }, ST ? SO.crc_mask : 0u, &passed);
            } else if (kList) {
                double bpm = shfld(stv[s].pm, gbase);
                for (int j = 1; j < L; ++j) {
                    const double pj = shfld(stv[s].pm, gbase + j);
                    if (pj < bpm) {  // first minimum (H6)
                        bpm = pj;
                        best = j;
                    }
                }
            }
            const int src = gbase + best;
            const int wsh = __builtin_ctz(wpl > 0 ? wpl : 1);
            if (split) {
                uint32_t x[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) x[k] = k < wpl ? polar_word(M.ldv(rl, r0 + gl * wpl + k, src)) : 0u;
#pragma unroll
                for (int mw = 1; mw < 8; mw *= 2)  // word stages inside the lane
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (!(k & mw) && k + mw < wpl) x[k] ^= x[k + mw];
                for (int lm = 1; lm < gs; lm <<= 1)  // word stages across the frame's lanes
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (k < wpl) {
                            const uint32_t o = (uint32_t)lane_read((int)x[k], lane ^ lm);
                            if (!(gl & lm)) x[k] ^= o;
                        }
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (k < wpl) M.lds[M.rw(k) + lane] = x[k];  // word gl*wpl + k at row k, column lane
                wave_sync();
            }
            const int64_t frame = (task * NS + s) * fpw + lane / gs;
            if constexpr (ST) {  // the output path's own metric and verdict, by the group's first lane
                const double wpm = shfld(stv[s].pm, src);
                if (gl == 0 && frame < B) {
                    if (SO.st_metric) SO.st_metric[frame] = wpm;
                    if (SO.st_pass) SO.st_pass[frame] = (uint8_t)passed;
                }
            }
            if (frame < B) {
                auto bit = [&](int pos) {
                    const int w = pos >> 5;
                    const uint32_t x = split ? M.lds[M.rw(w & (wpl - 1)) + gbase + (w >> wsh)] : M.ldv(rl, r0 + w, src);
                    return (x >> (pos & 31)) & 1u;
                };
                if (dword_out) {
                    // Four output bytes per store; 4 stores' loads issued together.
                    uint32_t *o32 = (uint32_t *)(out + frame * P.out_k);
                    const int nc = P.out_k >> 2;
                    for (int c0 = gl; c0 < nc; c0 += 4 * gs) {
                        uint32_t wv[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const int c = c0 + k * gs;
                            wv[k] = 0;
                            if (c < nc) {
                                const int4 pp = *(const int4 *)(P.info_pos + 4 * c);
                                wv[k] = bit(pp.x) | (bit(pp.y) << 8) | (bit(pp.z) << 16) | (bit(pp.w) << 24);
                            }
                        }
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (c0 + k * gs < nc) o32[c0 + k * gs] = wv[k];
                    }
                } else {
                    for (int t = gl; t < P.out_k; t += gs) out[frame * P.out_k + t] = (uint8_t)bit(P.info_pos[t]);
                }
            }
            if (split) wave_sync();  // the LDS rows are reused by the next set / task
        }
        wave_sync();
#ifdef QPD_STAMPS
        __builtin_amdgcn_s_waitcnt(0);
        if (threadIdx.x == 31) stamp_acc += __builtin_amdgcn_s_memtime() - stamp_t2;  // class 31: frame tail
        if (threadIdx.x == 31) stamp_cnt += 1;
        if (threadIdx.x < 32) {
            atomicAdd(&P.stamps[threadIdx.x], (unsigned long long)stamp_acc);
            atomicAdd(&P.stamps[32 + threadIdx.x], (unsigned long long)stamp_cnt);
        }
#endif
    }
}

// ---------------------------------------------------------------------------
// Frozen prefix (SCL-LUT in pre-mode): lut_fast_kernel<KIND, NS, false, false, true>.  Up to the first information leaf
// every path of a frame holds the same rows -- path 0 is the only one with a
// finite metric and all decisions are frozen zeros -- and until the third one
// at most 4 paths are live, yet the decode kernel would compute all of it L
// times (SCLLUTDecoder.cpp:62-144).  Two launches of this instantiation run
// that part of the schedule on the same op code and row layout:
//  * stage 1 -- the ops before the first forking op, one lane per frame (gs = 1,
//    64 frames per set);
//  * stage 2 -- from there to the op of the third information leaf at L = 4
//    (gs = 4), starting from stage 1's records (OP_IMPORT, MF_XBUF).
// Each stage ends with OP_EXPORT ops that write the rows the rest of the
// schedule reads before writing, through each path's lineage pointers, plus
// every path's metric, into the stage's own record buffer (qpd_decoder::pfx in
// qpd_capi.hip), interleaved across the frames of a 64-word block (FastPlan::pfx:
// address, record length and geometry).  The next stage or the decode kernel
// starts at the op after the split with OP_IMPORT ops (record address and
// layout in the op record) that copy each live path's record into its own
// column, zero the prefix's partial-sum rows (MF_ZERO) and load the metrics
// (MF_PM); dead slots start from path 0's rows with +inf.  The metrics are
// accumulated by the same code in the same leaf order, so the doubles are
// identical.
// ---------------------------------------------------------------------------
#define lut_prefix_kernel(KIND, NS, PW1) lut_fast_kernel<KIND, NS, false, false, true, PW1>

}  // namespace qpd
