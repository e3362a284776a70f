// qpd_fast_select.hpp -- the list decoders' path state and forks on the fast
// engine: the 2L -> L survivor selection of L = 8 (identity test keep_all8; the
// selection itself is qpd_common.hpp's select_survivors8) and of L = 9..16 (W16:
// keep_all16, select_survivors16), and the leaf forks built on them.  Needs no
// plan: tests/native/sel_harness.hip includes this header alone.
#pragma once
#include "qpd_fast_switches.hpp"

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qpd_common.hpp"
#include "stl_sort.hpp"

namespace qpd {

// ---------------------------------------------------------------------------
// List state and the fork (mink, SCLLUTDecoder.cpp:105-144).
//
// A wave runs NS independent frame sets through the same op stream.  The op
// records, the per-node tables and all scalar control are shared; the sets'
// dependency chains (LDS lookups, survivor selection, fork shuffles) are
// independent and interleave, which hides the LDS latency that bounds a
// single set.
// ---------------------------------------------------------------------------
// A path's metric and slot pointers: ps holds the S-row pointer fields, pu
// the U-row ones.  PW1: the host packed every field the op list uses into one
// word (at most 16 of them: SCL-LUT up to N = 2048, qpd_capi.hip:
// compact_pointer_fields), so U() is the same word -- two registers and two
// shuffles per fork less per frame set.
template <bool PW1>
struct PathT;
template <>
struct PathT<false> {
    double pm;
    uint64_t ps, pu;
    __device__ __forceinline__ uint64_t &U() { return pu; }
    __device__ __forceinline__ void move(int p) {  // take lane p's pointers (a fork)
        ps = shfl64(ps, p);
        pu = shfl64(pu, p);
    }
};
template <>
struct PathT<true> {
    double pm;
    uint64_t ps;
    __device__ __forceinline__ uint64_t &U() { return ps; }
    __device__ __forceinline__ void move(int p) { ps = shfl64(ps, p); }
};

// Move every set's state one slot down (set s + 1 into slot s, slot 0 to the
// end): a loop over the sets that runs set s in slot 0 has its own state back
// in place after NS steps.
template <class T, int NS>
__device__ __forceinline__ void rotate_sets(T (&a)[NS]) {
    if constexpr (NS > 1) {
        T t = a[0];
#pragma unroll
        for (int i = 0; i + 1 < NS; ++i) a[i] = a[i + 1];
        a[NS - 1] = t;
    }
}
template <class T, int NS, int W>
__device__ __forceinline__ void rotate_sets(T (&a)[NS][W]) {
#pragma unroll
    for (int w = 0; w < W; ++w) {
        T c[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) c[i] = a[i][w];
        rotate_sets(c);
#pragma unroll
        for (int i = 0; i < NS; ++i) a[i][w] = c[i];
    }
}

// max of two non-negative doubles given as bits (one v_max_f64).
__device__ __forceinline__ uint64_t dmax_bits(uint64_t a, uint64_t b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(__builtin_bit_cast(double, a)), "v"(__builtin_bit_cast(double, b)));
    return __builtin_bit_cast(uint64_t, r);
}

// max(-x, 0) in one v_max_f64 (the builtin would canonicalize its operand first).
__device__ __forceinline__ double neg_max0(double x) {
    double r;
    asm("v_max_f64 %0, -%1, 0" : "=v"(r) : "v"(x));
    return r;
}

// Identity test of the L = 8 survivor selection, for every lane group of the
// wave at once: the keeps K_j (this lane's keep key) are already in stable
// order (K_0 <= ... <= K_7) and no flip F_j beats the largest keep (a flip
// equal to a keep loses the tie: its candidate index is higher).  The stable
// sort of the 16 candidates then puts keep_j in slot j -- nothing moves and
// no flip survives.  Keys are >= +0 or +inf, never NaN (a NaN metric raises
// ERR_NAN_PM in the generic engine; LUT quanta are finite): max over doubles =
// max over their bits.  v_max_f64 by inline asm: the builtin would
// canonicalize the DPP operands first (two more VALU per step).
//
// First a conservative test on the high words alone (sign, exponent and the
// top 20 mantissa bits; keys are >= +0, so a larger high word is a larger
// double): strictly increasing keeps and every flip strictly above the
// largest keep's high word imply the identity.  32-bit words take the DPP
// lane moves inside the max / compare instructions (one VALU per step instead
// of two moves and a v_max_f64); only when it cannot decide (equal high words:
// near-ties) does the exact 64-bit test run.
template <int CTRL>
__device__ __forceinline__ uint32_t dpp32(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, CTRL, 0xF, 0xF, true);
}

__device__ __forceinline__ bool keep_all8(uint64_t K, uint64_t F, int gl) {
#if defined(QPD_EXP_IDENT)  // timing experiments only (wrong results): every selection the identity / none
    return QPD_EXP_IDENT;
#endif
#ifdef QPD_HI_IDENT  // measured -0.5 % on SCL-LUT (r04e): off
    {
        const uint32_t kh = (uint32_t)(K >> 32), fh = (uint32_t)(F >> 32);
        uint32_t m = kh;
        m = max(m, dpp32<kDppXor1>(m));
        m = max(m, dpp32<kDppXor2>(m));
        m = max(m, dpp32<kDppHalfMirror>(m));
        const uint32_t khn = dpp32<kDppRowShl1>(kh);
        // lanes with gl == 7 (every 8th) have no next slot: their sortedness bit is set
        const uint64_t up = __builtin_amdgcn_ballot_w64(fh > m);
        const uint64_t srt = __builtin_amdgcn_ballot_w64(khn > kh) | 0x8080808080808080ull;
        if ((up & srt) == ~0ull) return true;
    }
#endif
#ifndef QPD_IDENT_MAX  // the group maximum by a 3-step DPP reduction (round 3): 1.1 % slower (r04q)
    // With the keeps in order the largest is slot 7's, so no reduction: lanes
    // 4-7 of each group take K_7 (quad broadcast) and the flips of slots 7-4
    // (own) and 3-0 (half-row mirror) and compare both -- three independent
    // lane moves instead of a dependent max chain.  (Unordered keeps fail the
    // order ballot whatever K_7 is.)
    const uint64_t k7 = dpp64<kDppQuadBcast3>(K);
    const uint64_t fm = dpp64<kDppHalfMirror>(F);
    const uint64_t Kn = dpp64<kDppRowShl1>(K);  // keep of slot gl+1
    (void)gl;
    const uint64_t up = (__builtin_amdgcn_ballot_w64(F >= k7) & __builtin_amdgcn_ballot_w64(fm >= k7)) | 0x0F0F0F0F0F0F0F0Full;
    return (up & (__builtin_amdgcn_ballot_w64(K <= Kn) | 0x8080808080808080ull)) == ~0ull;
#else
    uint64_t mk = K;
    mk = dmax_bits(mk, dpp64<kDppXor1>(mk));
    mk = dmax_bits(mk, dpp64<kDppXor2>(mk));
    mk = dmax_bits(mk, dpp64<kDppHalfMirror>(mk));  // lane i^7 lies in the other quad
    const uint64_t Kn = dpp64<kDppRowShl1>(K);       // keep of slot gl+1
    (void)gl;
    return (__builtin_amdgcn_ballot_w64(F >= mk) & (__builtin_amdgcn_ballot_w64(K <= Kn) | 0x8080808080808080ull)) == ~0ull;
#endif
}

// ---------------------------------------------------------------------------
// List sizes 9..16 (LM = 16: lane groups of 16 = one DPP row, 4 frames per
// set).  mink (SCLLUTDecoder.cpp:8-21) sorts 2L > 16 candidates, so libstdc++
// runs its introsort, which is NOT stable: with tied keys the survivors' order
// is whatever the partitions leave (H1).  Without ties every correct sort
// gives the same first L outputs, so the kernel ranks by counting and replays
// the introsort only for a group whose first L ranks hold a tie:
//  * strict identity (keep_all16): keeps strictly increasing, every flip
//    strictly above the largest keep -- the unique sorted order puts keep j in
//    slot j whatever the algorithm;
//  * select_survivors16: dense key ranks against the 15 row partners by DPP
//    row rotations, then every group replays libstdc++'s partitions
//    (stl::partition_prefix, stl_sort.hpp) on its 2L ranks in parallel (scan-stop
//    masks, all of a partition's swaps at once); only a group that reaches the
//    introsort's depth limit replays stl::sort_small_prefix serially on its first lane.
// Candidates are encoded keep j -> j, flip j -> 16 + j (flips after keeps, as
// the reference's indices j < L <= L + j); lanes gl >= L are padding (+inf
// keys, never scattered below L).
// ---------------------------------------------------------------------------
template <int R>
__device__ __forceinline__ uint32_t dpp_ror(uint32_t x) {  // rotate within a row of 16 lanes
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x120 + R, 0xF, 0xF, false);
}
template <int R>
__device__ __forceinline__ uint64_t dpp_ror64(uint64_t x) {
    return ((uint64_t)dpp_ror<R>((uint32_t)(x >> 32)) << 32) | dpp_ror<R>((uint32_t)x);
}

__device__ __forceinline__ bool keep_all16(uint64_t K, uint64_t F, int gl, int gbase, int L) {
    const uint64_t Kn = dpp64<kDppRowShl1>(K);  // keep of slot gl + 1
    const uint64_t kl = shfl64(K, gbase + L - 1);
    const bool ok = (gl >= L - 1 || K < Kn) && (gl >= L || F > kl);
    return __builtin_amdgcn_ballot_w64(!ok) == 0;
}

// Dense key ranks: how many of the group's candidates have a strictly smaller
// key than this lane's keep / flip, counted against the 15 row partners (DPP
// row rotations).  lt preserves the order of the keys among the 2L
// candidates exactly (x < y <=> lt_x < lt_y), so the introsort replay below
// compares 5-bit ranks instead of doubles.  Padding lanes carry +inf: never
// smaller than anything.
template <int R>
__device__ __forceinline__ void lt16_all(uint64_t K, uint64_t F, int &lk, int &lf) {
    if constexpr (R < 16) {
        const uint64_t ok = dpp_ror64<R>(K), of = dpp_ror64<R>(F);
        lk += ok < K;
        lk += of < K;
        lf += ok < F;
        lf += of < F;
        lt16_all<R + 1>(K, F, lk, lf);
    }
}

// Index array of the serial replay in LDS (stl_sort.hpp Seq): keys by reference index.
struct SelReplay16 {
    int *idx;
    const double *key;
    __device__ int get(int p) { return idx[p]; }
    __device__ void set(int p, int e) { idx[p] = e; }
    __device__ bool less(int a, int b) { return key[a] < key[b]; }
};

// The group's array of 2L entries (lt << 5 | reference index), position p in
// lane p (p < L) or lane p - L (p >= L, upper half-word): every lane holds
// its keep's and its flip's starting positions.  w16_rd: the entry at a
// group-uniform position (a ds_bpermute: the whole wave executes it);
// w16_wr: this lane's word with that position's entry replaced.
__device__ __forceinline__ uint32_t w16_rd(uint32_t E, int gbase, int L, int p) {
    const bool hi = p >= L;
    const uint32_t w = (uint32_t)__builtin_amdgcn_ds_bpermute((gbase + (hi ? p - L : p)) << 2, (int)E);
    return hi ? w >> 16 : w & 0xFFFFu;
}
__device__ __forceinline__ uint32_t w16_wr(uint32_t E, int gl, int L, int p, uint32_t e) {
    const bool hi = p >= L;
    if (gl != (hi ? p - L : p)) return E;
    return hi ? (E & 0xFFFFu) | (e << 16) : (E & 0xFFFF0000u) | e;
}

// The group's mask of positions (bit p) whose flag is set, from the lanes'
// flags for their two positions (ballots; every lane gets its group's mask).
__device__ __forceinline__ uint32_t w16_mask(bool c0, bool c1, int gbase, int L) {
    const uint64_t b0 = __builtin_amdgcn_ballot_w64(c0), b1 = __builtin_amdgcn_ballot_w64(c1);
    const uint32_t m = (1u << L) - 1u;
    return ((uint32_t)(b0 >> gbase) & m) | (((uint32_t)(b1 >> gbase) & m) << L);
}

// Ranks of this lane's two packed u16 composites against the row partners' (R..15 lanes away).
template <int R, class LessM, class V>
__device__ __forceinline__ void rank16_packed(uint32_t X, LessM &lessm, V &acc) {
    if constexpr (R < 16) {
        const uint32_t Y = dpp_ror<R>(X);
        acc += lessm(__builtin_bit_cast(V, Y));
        acc += lessm(__builtin_bit_cast(V, __builtin_amdgcn_alignbit(Y, Y, 16)));
        rank16_packed<R + 1>(X, lessm, acc);
    }
}

// kDiag (the selection harness of tests/native/sel_harness.hip only): the lane groups
// whose bit (gbase / 16) is set in `serial_groups` take the serial replay from the
// start, beside groups that run the parallel one.  The decode kernels use the default:
// the mask is not read and the branch compiles out.
template <bool kDiag = false>
__device__ __forceinline__ Sel select_survivors16(double kk, double kf, int gl, int gbase, int L, int lane, int *sel,
                                                  int sj, uint32_t serial_groups = 0) {
    const uint64_t kInfBits = 0x7ff0000000000000ull;
    const bool pad = gl >= L;
    const uint64_t K = pad ? kInfBits : __builtin_bit_cast(uint64_t, kk);
    const uint64_t F = pad ? kInfBits : __builtin_bit_cast(uint64_t, kf);
    int lk = F < K, lf = K < F;
    lt16_all<1>(K, F, lk, lf);
    uint32_t E = pad ? 0xFFFFFFFFu : (((uint32_t)lk << 5) | (uint32_t)gl) | ((((uint32_t)lf << 5) | (uint32_t)(L + gl)) << 16);
    // stl::partition_prefix(seq, 0, 2L, L) replayed by each group on its array
    // (libstdc++ __introsort_loop's partitions, stl_sort.hpp): group-uniform f,
    // l, depth limit and end in every lane of the group.
    const int n2 = 2 * L;
    int f = 0, l = n2, dl = 2 * stl::lg(n2), end = n2;
    bool live = true, serial = false;
    if constexpr (kDiag) {
        serial = (serial_groups >> (gbase >> 4)) & 1u;
        live = !serial;
    }
#pragma unroll 1
    while (__builtin_amdgcn_ballot_w64(live)) {
        if (live && dl == 0) {  // heap-sort fallback: the group replays serially below
            serial = true;
            live = false;
        }
        --dl;
        const int mid = f + (l - f) / 2;
        // move_median_to_first(f, f + 1, mid, l - 1) on the ranks
        const uint32_t ea = w16_rd(E, gbase, L, f + 1), eb = w16_rd(E, gbase, L, mid), ec = w16_rd(E, gbase, L, l - 1);
        const uint32_t ef = w16_rd(E, gbase, L, f);
        const uint32_t ra = ea >> 5, rb = eb >> 5, rc = ec >> 5;
        int pick;
        if (ra < rb) pick = rb < rc ? mid : ra < rc ? l - 1 : f + 1;
        else pick = ra < rc ? f + 1 : rb < rc ? l - 1 : mid;
        const uint32_t em = pick == mid ? eb : pick == f + 1 ? ea : ec;
        if (live) {
            E = w16_wr(E, gl, L, f, em);
            E = w16_wr(E, gl, L, pick, ef);
        }
        // unguarded_partition(f + 1, l, pivot f): the left scan stops at ranks >= the
        // pivot's, the right scan at ranks <= it.  A swap leaves the untouched
        // positions as they were, so the k-th stops are the k-th such positions of
        // the array before the partition (from the left / from the right) while they
        // have not crossed; the scan that then runs on stops at the last right stop
        // at the latest (its swapped-in entry): cut = min(next left stop, last right stop).
        // All swaps at once: every stop position learns its rank among the left /
        // right stops (popcounts of the masks), publishes itself in the group's byte
        // slots (left stops at [0, 32), right stops at [32, 64) of the set's selection
        // scratch) and reads the stop of the same rank on the other side: the k-th pair
        // swaps iff its left stop lies below its right stop (a prefix of the k), and a
        // position is in at most one swapping pair.
        const uint32_t pv = em >> 5;
        const uint32_t in = ((l < 32 ? (1u << l) : 0u) - 1u) & ~((2u << f) - 1u);  // positions [f + 1, l)
        const uint32_t r0 = (E & 0xFFFFu) >> 5, r1 = E >> 21;
        const uint32_t GE = w16_mask(!pad && r0 >= pv, !pad && r1 >= pv, gbase, L) & in;
        const uint32_t LE = w16_mask(!pad && r0 <= pv, !pad && r1 <= pv, gbase, L) & in;
        uint8_t *const slot = (uint8_t *)sel + 4 * gbase;  // the group's 64 bytes
        const int q[2] = {gl, L + gl};
        int kA[2], kB[2];
        bool ge[2], le[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            ge[h] = !pad && ((GE >> q[h]) & 1u);
            le[h] = !pad && ((LE >> q[h]) & 1u);
            kA[h] = __builtin_popcount(GE & ((1u << q[h]) - 1u));                      // rank from the left
            kB[h] = __builtin_popcount(LE & ~((q[h] < 31 ? (2u << q[h]) : 0u) - 1u));  // rank from the right
            if (live && ge[h]) slot[kA[h]] = (uint8_t)q[h];
            if (live && le[h]) slot[32 + kB[h]] = (uint8_t)q[h];
        }
        lds_order();
        const int nA = __builtin_popcount(GE), nB = __builtin_popcount(LE);
        int part[2];
        bool lsw[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            part[h] = q[h];
            lsw[h] = false;
            const int bk = ge[h] && kA[h] < nB ? slot[32 + kA[h]] : -1;  // this left stop's right partner
            const int ak = le[h] && kB[h] < nA ? slot[kB[h]] : 64;       // this right stop's left partner
            if (q[h] < bk) {
                part[h] = bk;
                lsw[h] = true;
            } else if (ak < q[h]) {
                part[h] = ak;
            }
        }
        const int S = __builtin_popcount(w16_mask(lsw[0], lsw[1], gbase, L));  // swaps of this partition
        const int cut_a = S < nA ? slot[S] : n2, cut_b = S >= 1 ? slot[32 + S - 1] : n2;
        lds_order();
        const uint32_t x0 = w16_rd(E, gbase, L, part[0]), x1 = w16_rd(E, gbase, L, part[1]);
        if (live && !pad) E = x0 | (x1 << 16);
        if (live) {
            const int cut = cut_a < cut_b ? cut_a : cut_b;
            if (cut >= L && cut < end) end = cut;  // a block boundary past the first L positions
            if (l - cut > stl::kThreshold) {
                if (cut >= end) live = false;  // the reference's recursion on [cut, l) lies past the prefix
                else f = cut;
            } else {
                l = cut;
            }
            live = live && l - f > stl::kThreshold;
        }
    }
    // The final insertion sort of [0, end) is stable on the positions the partitions
    // left: its first L outputs are the L smallest (rank, position) -- ranks of the
    // composites (lt << 5 | position) counted against the row partners, packed u16.
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    const uint32_t p0 = (uint32_t)gl, p1 = (uint32_t)(L + gl);
    const uint32_t c0 = !pad && (int)p0 < end ? ((E & 0xFFE0u) | p0) : 0xFFFFu;
    const uint32_t c1 = !pad && (int)p1 < end ? (((E >> 16) & 0xFFE0u) | p1) : 0xFFFFu;
    const u16x2 X = __builtin_bit_cast(u16x2, c0 | (c1 << 16));
    const u16x2 one = {1, 1};
    auto lessm = [&](u16x2 y) { return __builtin_elementwise_min(__builtin_elementwise_sub_sat(X, y), one); };  // 1: y < x
    u16x2 R = lessm(__builtin_bit_cast(u16x2, __builtin_amdgcn_alignbit(c0 | (c1 << 16), c0 | (c1 << 16), 16)));
    rank16_packed<1>(c0 | (c1 << 16), lessm, R);
    const int rk0 = R.x, rk1 = R.y;
    const uint32_t cand0 = E & 31u, cand1 = (E >> 16) & 31u;
    sel[rk0 < L && !pad ? gbase + rk0 : sj + lane] = (int)(cand0 < (uint32_t)L ? cand0 : cand0 - L + 16);
    sel[rk1 < L && !pad ? gbase + rk1 : sj + lane] = (int)(cand1 < (uint32_t)L ? cand1 : cand1 - L + 16);
    lds_order();
    int c = pad ? gl : sel[gbase + gl];
    lds_order();
    const uint64_t slow = __builtin_amdgcn_ballot_w64(serial);
    if (slow) {
        // groups that reached the depth limit (heap-sort fallback), one after the other:
        // the whole replay on the group's first lane, keys by reference index at sel
        // (2L <= 32 doubles), the index array at the junk slots (2L ints)
        double *key = (double *)sel;
        int *idx = sel + sj;
#pragma unroll 1
        for (int g = 0; g < 64; g += 16) {
            if (!((slow >> g) & 0xFFFFull)) continue;
            if (gbase == g && !pad) {
                key[gl] = kk;
                key[L + gl] = kf;
            }
            lds_order();
            if (lane == g) {
                SelReplay16 seq{idx, key};
                for (int p = 0; p < 2 * L; ++p) idx[p] = p;
                stl::sort_small_prefix(seq, 0, 2 * L, L);  // libstdc++'s steps, first L outputs
            }
            lds_order();
            if (gbase == g && !pad) {
                const int e = idx[gl];
                c = e < L ? e : e - L + 16;
            }
            lds_order();
        }
    }
    Sel s;
    s.upper = c >= 16;
    s.parent = c & 15;
    return s;
}

// The one selection entry point of the list decoders' forks: keep key kk and
// flip key kf of this lane's path -> its slot's surviving candidate (parent,
// upper), as mink does on [keeps | flips] (SCLLUTDecoder.cpp:105-144 and
// FastSCLLUTDecoder.cpp:129, 187, 256, 332: every call site lays its 2L keys
// out as keep i at i, flip i at L + i, dead paths' +inf entries included).
// LM = 8: groups of 8 (DPP ranks), 16: L = 9..16 (the introsort replay), else
// the generic stable ranks of L <= 8.  fork_identity: the selection is known
// to be the identity in every group of the wave (never for the generic form).
template <int LM>
__device__ __forceinline__ bool fork_identity(double kk, double kf, int gl, int gbase, int L) {
    if constexpr (LM == 8) return keep_all8(__builtin_bit_cast(uint64_t, kk), __builtin_bit_cast(uint64_t, kf), gl);
    else if constexpr (LM == 16)
        return keep_all16(__builtin_bit_cast(uint64_t, kk), __builtin_bit_cast(uint64_t, kf), gl, gbase, L);
    else return false;
}
template <int LM>
__device__ __forceinline__ Sel fork_select(double kk, double kf, int gl, int gbase, int L, int lane, int *sel, int sj) {
    if constexpr (LM == 8) return select_survivors8(kk, kf, gl, gbase, lane, sel, sj);
    else if constexpr (LM == 16) return select_survivors16(kk, kf, gl, gbase, L, lane, sel, sj);
    else return select_survivors(kk, kf, gl, gbase, L, sel);
}

// Info leaf with quanta dm: keep the L best of {keep, flip} candidates.
// Returns the new decision; `extra` words follow the surviving lineage.
// `moved` (wave-uniform): the selection was not the identity (paths moved).
// LM: the list mode -- 8 (L = 8, groups of 8: DPP ranks), 16 (L = 9..16,
// groups of 16), 0 (L <= 8, the generic stable ranks).
template <int LM, int NX, class Path>
__device__ __forceinline__ uint32_t leaf_fork(Path &st, double dm, int gl, int gbase, int L, int lane, int *sel, int sj,
                                              uint32_t (&extra)[NX], bool &moved) {
    const double kf = st.pm + fabs(dm);
    const uint32_t hd = dm < 0;  // H4: SCL family `< 0`
    // Fast path (about 2/3 of the info leaves on the bench channel): the
    // selection is the identity, the decision the hard one.
    moved = false;
    if (fork_identity<LM>(st.pm, kf, gl, gbase, L)) return hd;
    moved = true;
    const Sel sl = fork_select<LM>(st.pm, kf, gl, gbase, L, lane, sel, sj);
    const int p = gbase + sl.parent;
    const uint32_t dec = (uint32_t)lane_read((int)hd, p) ^ (sl.upper ? 1u : 0u);
    st.pm = pick(sl.upper, shfld(kf, p), shfld(st.pm, p));
    st.move(p);
#pragma unroll
    for (int i = 0; i < NX; ++i) extra[i] = (uint32_t)lane_read((int)extra[i], p);
    return dec;
}

// One leaf decision for every set.  `frozen` is wave-uniform.
template <bool kList, int LM, int NS, int NX, class Path>
__device__ __forceinline__ void leaf_decide(Path (&st)[NS], const double (&dm)[NS], bool frozen, int gl, int gbase,
                                            int L, int lane, int *sel, int sstride, uint32_t (&extra)[NS][NX],
                                            uint32_t (&dec)[NS], bool (&moved)[NS]) {
#pragma unroll
    for (int s = 0; s < NS; ++s) moved[s] = false;
    if (!kList) {
#pragma unroll
        for (int s = 0; s < NS; ++s) dec[s] = frozen ? 0u : (uint32_t)(dm[s] <= 0);  // H4: SC family `<= 0`
        return;
    }
    if (frozen) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            // :100-104, |dm|·(dm<0) = max(-dm, 0): the same double (|dm|·1 = |dm| for
            // dm < 0; otherwise +0, or -0 for dm = +0, and pm + -0 = pm: pm is never -0)
            st[s].pm += neg_max0(dm[s]);
            dec[s] = 0u;
        }
        return;
    }
#pragma unroll
    for (int s = 0; s < NS; ++s)
        dec[s] = leaf_fork<LM>(st[s], dm[s], gl, gbase, L, lane, sel + sstride * s, NS * sstride, extra[s], moved[s]);
}

}  // namespace qpd
