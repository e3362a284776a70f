// qpd_fast_special.hpp -- the fast engine's special nodes (R0 / REP / SPC / R1):
// the R1 argsort with its introsort replay, the R1 layers, and the ops that run
// them for one frame set (special_op) or all of a wave's (r0rep_multi, r1_multi).
#pragma once
#include "qpd_fast_switches.hpp"

#include "qpd_fast_lookup.hpp"
#include "qpd_fast_select.hpp"

namespace qpd {

// ---------------------------------------------------------------------------
// Special nodes of the Fast decoders (FastSCLUT.cpp:46-107,
// FastSCLLUTDecoder.cpp:82-213).  The node's symbols are read a word (8
// symbols) at a time and their quanta vcl[d-1][pos][sym] (H3) fetched 8 at a
// time, so a node costs one memory round trip per 8 elements; sums still run
// in the reference's sequential element order (H5).
// ---------------------------------------------------------------------------

__device__ __forceinline__ uint32_t lomask(int x) { return x >= 32 ? 0xffffffffu : ((1u << x) - 1u); }
__device__ __forceinline__ uint32_t hibit(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); }  // x != 0

// stl::partition_prefix on an R1 array of 17..32 entries (keys < 16, MF_R1_RK),
// each Hoare partition driven by bit masks instead of its scans' dependent
// LDS reads: per round one pass over the array gives the positions whose key
// is >= / <= the pivot's; a partition's i-th left stop is then the next such
// position after the previous stop, or the previous right stop (whose
// swapped-in entry stops the scan there), the right stops likewise, and only
// the swaps touch LDS.  Returns `end` (partition_prefix); heap-sort fallbacks
// (the depth limit, never on the bench code) run stl::heap_sort as the
// reference does -- one lane's serial sort inside the ballot loop while the
// others go on partitioning.  tests/test_gpu_r1_nodes.py runs that branch on
// the device (tests/native/r1_harness.hip: the witnesses of
// tests/golden/r1_heap_witnesses.json in lanes beside arrays that partition to
// a natural end).
template <class Seq>
__device__ __forceinline__ int partition_prefix_masked(Seq &s, int temp, int m) {
    int f = 0, l = temp, dl = 0, end = temp;
    for (int t = temp; t > 1; t >>= 1) dl += 2;  // 2 * lg(temp)
    bool live = l - f > stl::kThreshold;
#pragma unroll 1
    while (__builtin_amdgcn_ballot_w64(live)) {
        if (live) {
            if (dl == 0) {
                stl::heap_sort(s, f, l);
                live = false;
            } else {
                --dl;
                stl::move_median_to_first(s, f, f + 1, f + (l - f) / 2, l - 1);
            }
        }
        // ranks >= / <= the pivot's over the 32 positions (one read pass)
        const uint32_t pv = (uint32_t)s.get(live ? f : 0) >> 5;
        uint32_t GE = 0u, LE = 0u;
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
            const uint32_t d = 2 * i < temp ? s.pair(i) : 0u;
            const uint32_t k0 = (d & 0xffffu) >> 5, k1 = d >> 21;
            GE |= ((uint32_t)(k0 >= pv) << (2 * i)) | ((uint32_t)(k1 >= pv) << (2 * i + 1));
            LE |= ((uint32_t)(k0 <= pv) << (2 * i)) | ((uint32_t)(k1 <= pv) << (2 * i + 1));
        }
        const uint32_t g0 = GE & lomask(l) & ~lomask(f + 1), e0 = LE & lomask(l) & ~lomask(f);
        uint32_t a = g0 ? (uint32_t)__builtin_ctz(g0) : 32u, b = e0 ? hibit(e0) : 0u;
        bool act = live && a < b;
#pragma unroll 1
        while (__builtin_amdgcn_ballot_w64(act)) {
            if (act) {
                const int ea = s.get((int)a), eb = s.get((int)b);
                s.set((int)a, eb);
                s.set((int)b, ea);
                const uint32_t in = lomask((int)b) & ~lomask((int)a + 1);
                const uint32_t g = GE & in, e = LE & in;
                const uint32_t na = g ? (uint32_t)__builtin_ctz(g) : b, nb = e ? hibit(e) : a;
                a = na;
                b = nb;
                act = a < b;
            }
        }
        if (live) {
            const int cut = (int)a;
            if (cut >= m && cut < end) end = cut;
            if (l - cut > stl::kThreshold) {
                if (cut >= end) live = false;
                else f = cut;
            } else {
                l = cut;
            }
            live = live && l - f > stl::kThreshold;
        }
    }
    return end;
}

// LDS view of the R1 argsort array: 16-bit entries (rank << 5 | element),
// entry p of this lane at row base + p/2, half p%2 of the lane's dword (rows
// `hs` halfwords apart: the set-interleaved row stride, see Mem).
struct LdsSeq16 {
    uint16_t *lane0;  // &row[base][lane] as 16-bit
    int hs;
    // entries 2i, 2i + 1 as one dword: a read that may alias the 16-bit stores
    // of set() (a plain uint32_t read may be moved above them: strict aliasing)
    __device__ __forceinline__ uint32_t pair(int i) const {
        typedef uint32_t __attribute__((may_alias)) u32a;
        return *(const u32a *)(lane0 + i * hs);
    }
    __device__ __forceinline__ int get(int p) const { return lane0[(p >> 1) * hs + (p & 1)]; }
    __device__ __forceinline__ void set(int p, int e) const { lane0[(p >> 1) * hs + (p & 1)] = (uint16_t)e; }
    __device__ __forceinline__ bool less(int a, int b) const { return (a >> 5) < (b >> 5); }  // keys only, as std::sort
};

// The argsort half of an R1 node of <= 32 elements (:100-116) for one set:
// the m smallest |l| in std::sort's order, packed for r1_layers -- ord[q] =
// element of the q-th smallest |llr| (5 bits each) and its symbol (4 bits
// each), hw = hard decisions (l < 0).  MAXM bounds the layers m = min(L - 1,
// temp): kMaxM = 7 (L <= 8: ordp0 holds 6 entries, ordp1 the seventh, symp all
// symbols) or 15 (L = 9..16: three order words of 6 entries, two symbol words of 8).
template <int MAXM>
struct R1PrepT;
template <>
struct R1PrepT<kMaxM> {
    uint32_t ordp0, ordp1, symp, hw;
    __device__ __forceinline__ int ord(int layer) const {
        return (int)(layer < 6 ? __builtin_amdgcn_ubfe(ordp0, 5 * layer, 5) : ordp1);
    }
    __device__ __forceinline__ uint32_t sym(int layer) const { return __builtin_amdgcn_ubfe(symp, 4 * layer, 4); }
    __device__ __forceinline__ void put(int q, int o, uint32_t sy) {
        symp |= sy << (4 * q);
        if (q < 6)
            ordp0 |= (uint32_t)o << (5 * q);
        else
            ordp1 = (uint32_t)o;
    }
};
template <>
struct R1PrepT<15> {
    uint32_t ordp0, ordp1, ordp2, symp0, symp1, hw;
    __device__ __forceinline__ int ord(int layer) const {
        const uint32_t w = layer < 6 ? ordp0 : layer < 12 ? ordp1 : ordp2;
        const int k = layer < 6 ? layer : layer < 12 ? layer - 6 : layer - 12;
        return (int)__builtin_amdgcn_ubfe(w, 5 * k, 5);
    }
    __device__ __forceinline__ uint32_t sym(int layer) const {
        return __builtin_amdgcn_ubfe(layer < 8 ? symp0 : symp1, 4 * (layer & 7), 4);
    }
    __device__ __forceinline__ void put(int q, int o, uint32_t sy) {  // q: a constant after unrolling
        (q < 8 ? symp0 : symp1) |= sy << (4 * (q & 7));
        (q < 6 ? ordp0 : q < 12 ? ordp1 : ordp2) |= (uint32_t)o << (5 * (q % 6));
    }
};
typedef R1PrepT<kMaxM> R1Prep;

// Survivor layers of an R1 node (FastSCLLUTDecoder.cpp:118-166) after its
// argsort (R1PrepT).  Each of the m layers forks on flipping the next element; the flip
// position is the slot's own pre-selection ord (H2).  The arrays never move: a
// slot's lineage holds the arrays its `origin` lane computed (read per layer
// by shuffles; each lane re-derives its own entry's magnitude, a quanta-row
// lookup or a vcl read), and its flips are one bit mask (temp <= 32) shuffled
// with the survivors.  Returns the node's bits.
template <int LM, int MAXM, class Path>
__device__ __forceinline__ uint32_t r1_layers(Path &st, int *sel, int sj, int gl, int gbase, int lane, int L, int m,
                                                     const R1PrepT<MAXM> &r, bool uni, double vrow, const double *vq, int v,
                                                     int temp) {
    const uint32_t hw = r.hw;
    uint32_t flips = 0;
    int origin = gl;
#if QPD_R1_UNROLL
#pragma unroll
#else
#pragma unroll 1  // (one copy of the fork code)
#endif
    for (int layer = 0; layer < MAXM; ++layer) {
        if (layer < m) {
            const int o = gbase + origin;
            const int own = r.ord(layer);
            const uint32_t sym = r.sym(layer);
            const double own_ms = fabs(uni ? shfld(vrow, (int)sym) : vq[(size_t)own * v + sym]);
            const double kf = st.pm + shfld(own_ms, o);
            // Identity selection in every group: no flip survives and no
            // lineage moves, and since each slot's magnitudes ascend with the
            // layer (argsort order) and pm + a is monotone in a, every later
            // layer's flips are at least as large -- all remaining layers are
            // the identity too, so the node is decided.  The same holds for the
            // STRICT identity of L = 9..16 (keep_all16: keeps strictly increasing,
            // every flip strictly above the largest keep): an identity layer leaves
            // the keeps as they are, and each slot's flip magnitudes are
            // non-decreasing with the layer, so flips strictly above the largest
            // keep stay strictly above it.
            if (fork_identity<LM>(st.pm, kf, gl, gbase, L)) break;
            const int pos_old = lane_read(own, o);  // H2
            const Sel sl = fork_select<LM>(st.pm, kf, gl, gbase, L, lane, sel, sj);
            const int p = gbase + sl.parent;
            st.pm = pick(sl.upper, shfld(kf, p), shfld(st.pm, p));
            st.move(p);
            origin = lane_read(origin, p);
            flips = (uint32_t)lane_read((int)flips, p) ^ (sl.upper ? 1u << (pos_old & 31) : 0u);
        }
    }
    const uint32_t word = (uint32_t)lane_read((int)hw, gbase + origin) ^ flips;
    return temp < 32 ? word & ((1u << temp) - 1u) : word;
}

// Word w of a special node's symbols: its S[d] row, or (MF_SFG, size-8 nodes)
// f / g (MF_SGG, u = the left sibling's U[d] through usrc) of its depth d-1
// parent's two words, with the parent's table T2 (staged as bytes at tb: LT).
template <bool LT>
__device__ __forceinline__ uint32_t spec_in(const Mem &M, const MOp &op, int src, int usrc, int w, uint32_t T2,
                                            const uint8_t *tb) {
    const bool sl = op.flags & MF_SRC_LDS;
    if (!(op.flags & MF_SFG)) return M.ld(sl, op.src_row + w, src);
    const uint32_t a = M.ld(sl, op.src_row, src), b = M.ld(sl, op.src_row + 1, src);
    const uint32_t ub = (op.flags & MF_SGG) ? M.ld(op.flags & MF_U_LDS, op.u_row, usrc) : 0u;
    return LT ? lut_lds<8, true>(a, b, ub) : lut_vec<8>(T2, a, b, ub);  // (f: ub = 0, entries < 256)
}

// A special node's result word(s) `res` to its destination; MF_SCOMB (size 8):
// the parent's combine with the left sibling's U[d] (through the path's
// pointer after the node's forks, as the COMB op would read it) instead, to
// the parent's destination (utils.cpp:62-67).
template <class Path>
__device__ __forceinline__ void spec_out(const Mem &M, const MOp &op, Path &st, int gbase, int gl, int lane, int w,
                                         uint32_t res) {
    if (op.flags & MF_SCOMB)
        res = ((M.ld(op.flags & MF_U_LDS, op.u_row, gbase + pfield(st.U(), op.sh_u)) & 0xFFu) ^ res) | (res << 8);
    M.st(op.flags & MF_DST_LDS, op.dst_row + w, lane, res);
}

// GEN = false (the FastSCL-LUT kernels without R1L): every R1 node has its ranks in
// the op record (MF_R1_RK, one quanta row) -- the host takes the R1L instantiation
// otherwise -- so the rank-table and std::sort paths are not compiled.
// MAXM: the layer bound (R1PrepT); both argsort paths deliver the first m <= MAXM outputs of
// std::sort -- <= 16 elements: its insertion sort is stable, the min-tree pick on (rank, element);
// 17..32: the partitions replayed in the LDS tail, then the m smallest (rank, position) of [0, end).
template <bool LT = false, bool GEN = true, int MAXM = kMaxM, class Path>
__device__ __forceinline__ R1PrepT<MAXM> r1_prep(const FastPlan &P, const Mem &M, const MOp &op, Path st, int gbase, int L,
                                          int lane, int temp, uint32_t *lds_wave, uint32_t T2 = 0u,
                                          const uint8_t *tb = nullptr) {
    const int src = gbase + pfield(st.ps, op.sh_src);
    const int v = P.v;
    const int m = (L - 1) < temp ? (L - 1) : temp;
    const uint16_t *rk = P.r1_rank + op.tab;
    const double *vq = P.vcl + (size_t)op.vrow * v;
    // MF_VUNI: one quanta row and one rank row for all elements, in registers
    const bool uni = !GEN || (op.flags & MF_VUNI), rku = !GEN || (op.flags & MF_R1_RK);
    const int s16 = lane & 15;
    const uint32_t rrow = GEN && uni && !rku && s16 < v ? (uint32_t)rk[s16] : 0u;
    (void)vq;
    // rank << 1 | sign of element j's symbol: from the op record's words (MF_R1_RK), the node's
    // one rank row in a register (MF_VUNI), or the per-element rank table
    const uint64_t RK = ((uint64_t)(uint32_t)op.tab2 << 32) | (uint32_t)op.r_row;
    auto rank_of = [&](int j, uint32_t sym) -> uint32_t {
        if (rku) return ((uint32_t)(RK >> (4 * sym)) & 15u) << 1 | (((uint32_t)op.pad1 >> sym) & 1u);
        return uni ? (uint32_t)lane_read((int)rrow, (int)sym) : (uint32_t)rk[j * v + sym];
    };
    uint32_t W[4], hw = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w)
        W[w] = (8 * w < temp) ? spec_in<LT>(M, op, src, gbase + pfield(st.U(), op.sh_u), w, T2, tb) : 0u;
    int ord[MAXM];
#pragma unroll
    for (int q = 0; q < MAXM; ++q) ord[q] = 0;
    if ((QPD_EXP_FSCL & 8) || temp <= stl::kThreshold) {
        // entries rank << 5 | j (< 2^14) two per register; the m smallest by
        // packed 16-bit min trees (v_pk_min_u16), the taken one set to 0xFFFF
        typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
        u16x2 ep[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            uint32_t lo = 0xffffu, hi = 0xffffu;
            if (2 * i < temp) {
                const uint32_t e = rank_of(2 * i, (W[i >> 2] >> (8 * (i & 3))) & 15u);
                hw |= (e & 1u) << (2 * i);
                lo = ((e >> 1) << 5) | (uint32_t)(2 * i);
            }
            if (2 * i + 1 < temp) {
                const uint32_t e = rank_of(2 * i + 1, (W[i >> 2] >> (8 * (i & 3) + 4)) & 15u);
                hw |= (e & 1u) << (2 * i + 1);
                hi = ((e >> 1) << 5) | (uint32_t)(2 * i + 1);
            }
            ep[i] = __builtin_bit_cast(u16x2, lo | (hi << 16));
        }
#pragma unroll
        for (int q = 0; q < MAXM; ++q) {
            if (q < m) {
                u16x2 a = __builtin_elementwise_min(__builtin_elementwise_min(ep[0], ep[1]),
                                                    __builtin_elementwise_min(ep[2], ep[3]));
                u16x2 b = __builtin_elementwise_min(__builtin_elementwise_min(ep[4], ep[5]),
                                                    __builtin_elementwise_min(ep[6], ep[7]));
                a = __builtin_elementwise_min(a, b);
                const uint32_t mn = a.x < a.y ? a.x : a.y;
                ord[q] = (int)(mn & 31u);
                const u16x2 mm = {(unsigned short)mn, (unsigned short)mn};
                const u16x2 one = {1, 1}, zero = {0, 0};
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const u16x2 d = ep[i] - mm;                                // 0 where taken (all entries >= mn)
                    const u16x2 t = __builtin_elementwise_min(d, one) ^ one;   // 1 where taken
                    ep[i] = ep[i] | (zero - t);                               // taken -> 0xFFFF
                }
            }
        }
    } else {
        // the wave's whole LDS tail from the sets' row u_row on (the rows of depths > d and the
        // selection scratch of every set: free while this node runs; the sets run one after the
        // other), one 64-lane row per two entries
        const LdsSeq16 seq{(uint16_t *)(lds_wave + M.rw(op.u_row) + lane), 128};
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            if (j < temp) {
                const uint32_t e = rank_of(j, (W[j >> 3] >> (4 * (j & 7))) & 15u);
                hw |= (e & 1u) << j;
                seq.set(j, (int)(((e >> 1) << 5) | (uint32_t)j));
            }
        }
        if (rku) {
            // the partitions in LDS, then the m smallest of the block [0, end) by (rank, position):
            // what the final insertion sort's first m outputs are (stl::partition_prefix), by
            // packed 16-bit min trees over rank << 10 | position << 5 | element (ranks < 16)
            const int end = QPD_EXP_FSCL & 128 ? stl::partition_prefix(seq, 0, temp, m) : partition_prefix_masked(seq, temp, m);
            typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
            u16x2 ep[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const uint32_t d = 2 * i < temp ? seq.pair(i) : 0u;  // entries 2i, 2i + 1
                const uint32_t e0 = d & 0xffffu, e1 = d >> 16;
                const uint32_t lo = 2 * i < end ? ((e0 >> 5) << 10) | ((uint32_t)(2 * i) << 5) | (e0 & 31u) : 0xffffu;
                const uint32_t hi = 2 * i + 1 < end ? ((e1 >> 5) << 10) | ((uint32_t)(2 * i + 1) << 5) | (e1 & 31u) : 0xffffu;
                ep[i] = __builtin_bit_cast(u16x2, lo | (hi << 16));
            }
#pragma unroll
            for (int q = 0; q < MAXM; ++q) {
                if (q < m) {
                    u16x2 a[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) a[i] = __builtin_elementwise_min(ep[2 * i], ep[2 * i + 1]);
#pragma unroll
                    for (int w = 4; w >= 1; w >>= 1)
#pragma unroll
                        for (int i = 0; i < w; ++i) a[i] = __builtin_elementwise_min(a[i], a[i + w]);
                    const uint32_t mn = a[0].x < a[0].y ? a[0].x : a[0].y;
                    ord[q] = (int)(mn & 31u);
                    const u16x2 mm = {(unsigned short)mn, (unsigned short)mn};
                    const u16x2 one = {1, 1}, zero = {0, 0};
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const u16x2 dd = ep[i] - mm;
                        ep[i] = ep[i] | (zero - (__builtin_elementwise_min(dd, one) ^ one));  // taken -> 0xFFFF
                    }
                }
            }
        } else if constexpr (GEN) {
            stl::sort_small_prefix(seq, 0, temp, m);  // only ord[0, m) is read
#pragma unroll
            for (int q = 0; q < MAXM; ++q)
                if (q < m) ord[q] = seq.get(q) & 31;
        }
    }
    R1PrepT<MAXM> r{};
    r.hw = hw;
#pragma unroll
    for (int q = 0; q < MAXM; ++q) {
        if (q < m) {
            const int k = ord[q] >> 3;
            const uint32_t w = k == 0 ? W[0] : k == 1 ? W[1] : k == 2 ? W[2] : W[3];
            r.put(q, ord[q], (w >> (4 * (ord[q] & 7))) & 15u);
        }
    }
    return r;
}

template <int LM, class Path>
__device__ __forceinline__ void r1_small(const FastPlan &P, const Mem &M, const MOp &op, Path &st, int *sel, int sj,
                                         int gl, int gbase, int L, int lane, int temp, uint32_t *lds_wave) {
    const int v = P.v;
    const int m = (L - 1) < temp ? (L - 1) : temp;
    const double *vq = P.vcl + (size_t)op.vrow * v;
    const bool uni = op.flags & MF_VUNI;
    const double vrow = uni && (lane & 15) < v ? vq[lane & 15] : 0.0;
    constexpr int MAXM = LM == 16 ? 15 : kMaxM;
    // (LM = 16: the argsort is done with the LDS tail -- order, symbols and hard decisions are in
    // registers -- before the first layer's selection writes the scratch inside it)
    const R1PrepT<MAXM> r = r1_prep<false, true, MAXM>(P, M, op, st, gbase, L, lane, temp, lds_wave);
    const uint32_t word = r1_layers<LM, MAXM>(st, sel, sj, gl, gbase, lane, L, m, r, uni, vrow, vq, v, temp);
    M.st(op.flags & MF_DST_LDS, op.dst_row, lane, word);
}

// R1 nodes of <= 32 elements with L = 8 for all the wave's frame sets: the
// argsorts set by set, then the layers of the sets interleaved (their fork
// chains overlap), each set stopping at its first identity layer (r1_layers).
template <bool LT, bool GEN, int NS, class Path>
__device__ __forceinline__ void r1_multi(const FastPlan &P, const Mem (&Mv)[NS], const MOp &op, Path (&st)[NS], int *sel_all,
                                         int sstride, int gl, int gbase, int lane, uint32_t *lds_wave, uint32_t T2,
                                         uint8_t *tb) {
    const int temp = op.cnt, v = P.v;
    const int m = kMaxM < temp ? kMaxM : temp;  // L = 8
    const double *vq = P.vcl + (size_t)op.vrow * v;
    const bool uni = !GEN || (op.flags & MF_VUNI);
    const double vrow = uni && (lane & 15) < v ? vq[lane & 15] : 0.0;
    if constexpr (LT)
        if (op.flags & MF_SFG) stage_tab(tb, T2, (op.flags & MF_SGG) ? gtab_dw(lane) : (lane & 31));
    R1Prep pr[NS];
#pragma unroll 1
    for (int s = 0; s < NS; ++s) {  // set s in slot 0 (rotate_sets)
        if ((QPD_EXP_FSCL & 64) && temp > 16) pr[0] = R1Prep{0x1a418820u, 6u, 0u, 0u};  // (ord 0..6)
        else
        pr[0] = r1_prep<LT, GEN>(P, Mv[0].set(s), op, st[0], gbase, 8, lane, temp, lds_wave, T2, tb);
        rotate_sets(st);
        rotate_sets(pr);
    }
    uint32_t flips[NS];
    int origin[NS];
    bool done[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        flips[s] = 0;
        origin[s] = gl;
        done[s] = false;
    }
#pragma unroll 1
    for (int layer = 0; layer < ((QPD_EXP_FSCL & 32) && temp > 16 ? 0 : m); ++layer) {
        double kf[NS];
        int own[NS];
        bool all = true;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (done[s]) continue;
            const int o = gbase + origin[s];
            own[s] = (int)(layer < 6 ? __builtin_amdgcn_ubfe(pr[s].ordp0, 5 * layer, 5) : pr[s].ordp1);
            const uint32_t sym = __builtin_amdgcn_ubfe(pr[s].symp, 4 * layer, 4);
            const double own_ms = fabs(!GEN || uni ? shfld(vrow, (int)sym) : vq[(size_t)own[s] * v + sym]);
            kf[s] = st[s].pm + shfld(own_ms, o);
            done[s] = keep_all8(__builtin_bit_cast(uint64_t, st[s].pm), __builtin_bit_cast(uint64_t, kf[s]), gl);
            all = all && done[s];
        }
        if (all) break;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (done[s]) continue;
            const int o = gbase + origin[s];
            const int pos_old = lane_read(own[s], o);  // H2
            const Sel sl = select_survivors8(st[s].pm, kf[s], gl, gbase, lane, sel_all + sstride * s, NS * sstride);
            const int p = gbase + sl.parent;
            st[s].pm = pick(sl.upper, shfld(kf[s], p), shfld(st[s].pm, p));
            st[s].move(p);
            origin[s] = lane_read(origin[s], p);
            flips[s] = (uint32_t)lane_read((int)flips[s], p) ^ (sl.upper ? 1u << (pos_old & 31) : 0u);
        }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        uint32_t word = (uint32_t)lane_read((int)pr[s].hw, gbase + origin[s]) ^ flips[s];
        if (temp < 32) word &= (1u << temp) - 1u;
        spec_out(Mv[s], op, st[s], gbase, gl, lane, 0, word);
        if (!(op.flags & MF_TO_R)) st[s].U() = pset(st[s].U(), op.sh_dst, gl);
    }
}

// R0 / REP nodes with L = 8 for all the wave's frame sets, interleaved element
// by element (their sums are dependent fp64 chains in the reference's order,
// H5; the sets' chains overlap).
// GEN = false (the FastSCL-LUT kernels without R1L): every R0 / REP node has one quanta
// row (MF_VUNI; the host takes the R1L instantiation otherwise).  With the byte-table
// slot (LT) the two sums' terms of each symbol, (l < 0)|l| and (l >= 0)|l|, are staged
// in it once per node and each element reads both with one ds_read_b128 (the same
// doubles as the selects on the quanta: the sums are unchanged).
template <bool LT, bool GEN, int NS, class Path>
__device__ __forceinline__ void r0rep_multi(const FastPlan &P, const Mem (&Mv)[NS], const MOp &op, Path (&st)[NS], int *sel_all,
                                            int sstride, int gl, int gbase, int lane, uint32_t T2, uint8_t *tb) {
    const int fl = op.flags, temp = op.cnt, v = P.v;
    const bool rep = op.type == OP_REP, sl = fl & MF_SRC_LDS, dl = fl & MF_DST_LDS;
    const double *vq = P.vcl + (size_t)op.vrow * v;  // row d-1, position temp*node
    const bool uni = !GEN || (fl & MF_VUNI);
    const double vr = uni && (lane & 15) < v ? vq[lane & 15] : 0.0;
    int src[NS];
    double kk[NS], kf[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        src[s] = gbase + pfield(st[s].ps, op.sh_src);
        kk[s] = kf[s] = st[s].pm;
    }
    const int n8 = (temp + 7) >> 3;
    if constexpr (LT)
        if (fl & MF_SFG) stage_tab(tb, T2, (fl & MF_SGG) ? gtab_dw(lane) : (lane & 31));
    typedef double d2 __attribute__((ext_vector_type(2)));
    d2 *const qt = (d2 *)(tb + 512);  // (LT, !GEN) the symbols' terms, after the f / g tables' 512 B
    if constexpr (LT && !GEN) {
        if (lane < 16) qt[lane] = d2{vr < 0 ? fabs(vr) : 0.0, vr >= 0 ? fabs(vr) : 0.0};
        lds_order();
    }
#pragma unroll 1
    for (int w = 0; w < n8; ++w) {
        uint32_t word[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) word[s] = spec_in<LT>(Mv[s], op, src[s], gbase + pfield(st[s].U(), op.sh_u), w, T2, tb);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            if (8 * w + i >= temp) break;
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                const uint32_t sym = (word[s] >> (4 * i)) & 15u;
                if constexpr (LT && !GEN) {
                    const d2 t = qt[sym];
                    kk[s] += t.x;
                    if (rep) kf[s] += t.y;
                    continue;
                }
                const double l = uni ? shfld(vr, (int)sym) : vq[(size_t)(8 * w + i) * v + sym];
                kk[s] += l < 0 ? fabs(l) : 0.0;  // :88-95 / :176-180, (l<0)·|l|, (l>=0)·|l| as selects
                if (rep) kf[s] += l >= 0 ? fabs(l) : 0.0;
            }
        }
    }
    if constexpr (LT && !GEN) lds_order();  // (the slot's next writer comes after these reads)
    const int nwo = (temp + 31) >> 5;
    const uint32_t m = temp < 32 ? ((1u << temp) - 1u) : 0xffffffffu;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        uint32_t fill = 0;
        if (!rep || keep_all8(__builtin_bit_cast(uint64_t, kk[s]), __builtin_bit_cast(uint64_t, kf[s]), gl)) {
            st[s].pm = kk[s];  // R0; REP: the identity selection, every path keeps its all-zeros codeword
        } else {
            const Sel sx = select_survivors8(kk[s], kf[s], gl, gbase, lane, sel_all + sstride * s, NS * sstride);
            const int p = gbase + sx.parent;
            st[s].pm = pick(sx.upper, shfld(kf[s], p), shfld(kk[s], p));
            st[s].move(p);
            fill = sx.upper ? 0xffffffffu : 0u;
        }
        for (int w = 0; w < nwo; ++w) spec_out(Mv[s], op, st[s], gbase, gl, lane, w, fill & m);
        if (!(fl & MF_TO_R)) st[s].U() = pset(st[s].U(), op.sh_dst, gl);
    }
}

// Per-lane argsort arrays (global scratch) for the R1 node; rows of this set
// (stride `rs` words, see Mem), a key's double as two rows (low, high word).
struct FastSortSeq {
    uint32_t *glb;
    int io, ko, lane, rs;
    __device__ int get(int p) { return (int)glb[(size_t)(io + p) * rs + lane]; }
    __device__ void set(int p, int e) { glb[(size_t)(io + p) * rs + lane] = (uint32_t)e; }
    __device__ double key(int e) {
        const uint64_t lo = glb[(size_t)(ko + 2 * e) * rs + lane], hi = glb[(size_t)(ko + 2 * e + 1) * rs + lane];
        return __builtin_bit_cast(double, lo | (hi << 32));
    }
    __device__ bool less(int a, int b) { return key(a) < key(b); }
};

// R1 nodes above 32 elements (N >= 2048 codes) or without LDS room: the
// argsort arrays live in the wave's global slab (H / K / I rows).
template <class Path>
__device__ __forceinline__ void r1_large(const FastPlan &P, const Mem &M, const MOp &op, Path &st, int *sel, int gl,
                                      int gbase, int L, int lane, int temp) {
    const int src = gbase + pfield(st.ps, op.sh_src);
    const bool sl = op.flags & MF_SRC_LDS, dl = op.flags & MF_DST_LDS;
    const int nwo = (temp + 31) >> 5;
    const double *vq = P.vcl + (size_t)op.vrow * P.v;
    auto llr = [&](int j) -> double {
        const uint32_t w = M.ld(sl, op.src_row + (j >> 3), src);
        return vq[(size_t)j * P.v + ((w >> ((j & 7) << 2)) & 15u)];
    };
    const int m = (L - 1) < temp ? (L - 1) : temp;
    uint32_t *g = M.gp;
    for (int w = 0; w < nwo; ++w) {
        uint32_t word = 0;
        for (int i = 0; i < 32 && 32 * w + i < temp; ++i) {
            const int j = 32 * w + i;
            const double l = llr(j);
            word |= (uint32_t)(l < 0) << i;
            const uint64_t b = __builtin_bit_cast(uint64_t, fabs(l));
            g[(size_t)M.rw(P.K_row + 2 * j) + lane] = (uint32_t)b;
            g[(size_t)M.rw(P.K_row + 2 * j + 1) + lane] = (uint32_t)(b >> 32);
        }
        g[(size_t)M.rw(P.H_row + w) + lane] = word;
    }
    int ord[kMaxM];
    double ms[kMaxM];
    int flip[kMaxM];
    for (int q = 0; q < kMaxM; ++q) {
        ord[q] = 0;
        ms[q] = 0;
        flip[q] = -1;
    }
    FastSortSeq seq{g, P.I_row, P.K_row, lane, M.ns * 64};
    for (int p = 0; p < temp; ++p) seq.set(p, p);
    stl::sort(seq, 0, temp);
    for (int q = 0; q < kMaxM; ++q) {
        if (q < m) {
            ord[q] = seq.get(q);
            ms[q] = seq.key(ord[q]);
        }
    }
    wave_sync();  // H rows visible to the whole wave
    int origin = gl;
    for (int layer = 0; layer < kMaxM; ++layer) {
        if (layer < m) {
            const double kf = st.pm + ms[layer];
            const Sel sx = select_survivors(st.pm, kf, gl, gbase, L, sel);
            const int p = gbase + sx.parent;
            const int pos_old = ord[layer];  // H2
            st.pm = pick(sx.upper, shfld(kf, p), shfld(st.pm, p));
            st.move(p);
            origin = lane_read(origin, p);
            for (int q = 0; q < kMaxM; ++q) {
                ord[q] = lane_read(ord[q], p);
                ms[q] = shfld(ms[q], p);
                if (q < layer) flip[q] = lane_read(flip[q], p);
            }
            flip[layer] = sx.upper ? pos_old : -1;
        }
    }
    for (int w = 0; w < nwo; ++w) {
        uint32_t word = g[(size_t)M.rw(P.H_row + w) + gbase + origin];
        for (int q = 0; q < kMaxM; ++q)
            if (q < m && flip[q] >= 0 && (flip[q] >> 5) == w) word ^= 1u << (flip[q] & 31);
        if (temp < 32) word &= (1u << temp) - 1u;
        M.st(dl, op.dst_row + w, lane, word);
    }
}

// R1L: the schedule has an R1 node that needs r1_large (> 32 elements, or > 16
// without LDS room; N >= 2048 codes).  Only those plans get it compiled in:
// its argsort stack and arrays cost the other instantiations registers and
// scratch (+3 % FastSCL-LUT at N = 1024 without it).
template <bool kList, int LM, bool R1L, class Path>
__device__ __forceinline__ void special_op(const FastPlan &P, const Mem &M, const MOp &op, Path &st, int *sel, int sj,
                                           int gl, int gbase, int L, int lane, uint32_t *lds_wave) {
    const int fl = op.flags;
    const int temp = op.cnt;
    const int src = gbase + pfield(st.ps, op.sh_src);
    const bool dl = fl & MF_DST_LDS, sl = fl & MF_SRC_LDS;
    const int nwo = (temp + 31) >> 5;
    const int v = P.v;
    const double *vq = P.vcl + (size_t)op.vrow * v;  // row d-1, position temp*node
    // MF_VUNI: the node's one quanta row, entry s in lanes s, s+16, s+32, s+48
    const bool uni = fl & MF_VUNI;
    const double vr = uni && (lane & 15) < v ? vq[lane & 15] : 0.0;
    // elements [8w, 8w + 8) of the node: quanta of its symbols
    auto llr8 = [&](int w, double (&l)[8], uint32_t &word) {
        word = M.ld(sl, op.src_row + w, src);
        if (uni) {
#pragma unroll
            for (int i = 0; i < 8; ++i) l[i] = shfld(vr, (int)((word >> (4 * i)) & 15u));
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i)
                l[i] = (8 * w + i < temp) ? vq[(size_t)(8 * w + i) * v + ((word >> (4 * i)) & 15u)] : 0.0;
        }
    };
    const int n8 = (temp + 7) >> 3;
    if (QPD_EXP_FSCL & 2) return;
    if (op.type == OP_R0) {
        if (kList) {
            for (int w = 0; w < n8; ++w) {
                double l[8];
                uint32_t word;
                llr8(w, l, word);
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (8 * w + i < temp) st.pm += l[i] < 0 ? fabs(l[i]) : 0.0;  // H5; (float)(l<0)·|l| as a select
            }
        }
        for (int w = 0; w < nwo; ++w) M.st(dl, op.dst_row + w, lane, 0u);
    } else if (op.type == OP_REP && !(QPD_EXP_FSCL & 16)) {
        uint32_t fill = 0;
        if (!kList) {
            double S = 0;
            for (int w = 0; w < n8; ++w) {
                double l[8];
                uint32_t word;
                llr8(w, l, word);
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (8 * w + i < temp) S += l[i];
            }
            fill = S <= 0 ? 0xffffffffu : 0u;  // H4
        } else {
            double kk = st.pm, kf = st.pm;
            for (int w = 0; w < n8; ++w) {
                double l[8];
                uint32_t word;
                llr8(w, l, word);
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (8 * w + i < temp) {
                        kk += l[i] < 0 ? fabs(l[i]) : 0.0;  // (l<0)·|l|, (l>=0)·|l| as selects
                        kf += l[i] >= 0 ? fabs(l[i]) : 0.0;
                    }
            }
            if (fork_identity<LM>(kk, kf, gl, gbase, L)) {
                st.pm = kk;  // identity selection: every path keeps its all-zeros codeword
            } else {
                const Sel sx = fork_select<LM>(kk, kf, gl, gbase, L, lane, sel, sj);
                const int p = gbase + sx.parent;
                st.pm = pick(sx.upper, shfld(kf, p), shfld(kk, p));
                st.move(p);
                fill = sx.upper ? 0xffffffffu : 0u;
            }
        }
        const uint32_t m = temp < 32 ? ((1u << temp) - 1u) : 0xffffffffu;
        for (int w = 0; w < nwo; ++w) M.st(dl, op.dst_row + w, lane, fill & m);
    } else if (op.type == OP_SPC) {  // FastSC only
        uint32_t parity = 0, word = 0;
        double best = 0;
        int bi = 0;
        for (int w = 0; w < n8; ++w) {
            double l[8];
            uint32_t sw;
            llr8(w, l, sw);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int j = 8 * w + i;
                if (j < temp) {
                    const uint32_t h = l[i] <= 0;
                    word |= h << (j & 31);
                    parity ^= h;
                    const double a = fabs(l[i]);
                    if (j == 0 || a < best) {  // first minimum (H6)
                        best = a;
                        bi = j;
                    }
                }
            }
            if ((w & 3) == 3 || w == n8 - 1) {
                M.st(dl, op.dst_row + (w >> 2), lane, word);
                word = 0;
            }
        }
        if (parity) {
            const int row = op.dst_row + (bi >> 5);
            M.stv(dl, row, lane, M.ldv(dl, row, lane) ^ (1u << (bi & 31)));  // bi: per lane
        }
    } else if (!kList) {  // OP_R1, FastSC: `<= 0`
        uint32_t word = 0;
        for (int w = 0; w < n8; ++w) {
            double l[8];
            uint32_t sw;
            llr8(w, l, sw);
#pragma unroll
            for (int i = 0; i < 8; ++i)
                if (8 * w + i < temp) word |= (uint32_t)(l[i] <= 0) << ((8 * w + i) & 31);
            if ((w & 3) == 3 || w == n8 - 1) {
                M.st(dl, op.dst_row + (w >> 2), lane, word);
                word = 0;
            }
        }
    } else if (QPD_EXP_FSCL & 4) {
    } else if (temp <= stl::kThreshold || (fl & MF_R1_LDS)) {
        r1_small<LM>(P, M, op, st, sel, sj, gl, gbase, L, lane, temp, lds_wave);
    } else if constexpr (R1L) {
        r1_large(P, M, op, st, sel, gl, gbase, L, lane, temp);
    }
    if (!(fl & MF_TO_R)) st.U() = pset(st.U(), op.sh_dst, gl);
}

}  // namespace qpd
