// qpd_fast_bot.hpp -- the fast engine's bottom subtrees of height 3, held in
// registers: BOT3 (bot_pair, bot3_op) and the mixed subtrees with FastSCL special
// nodes of size 4 / 2 (BOTX: bx_spec, bx_spec_multi, bx_load, botx_op).
#pragma once
#include "qpd_fast_switches.hpp"

#include "qpd_fast_lookup.hpp"
#include "qpd_fast_select.hpp"

namespace qpd {

// ---------------------------------------------------------------------------
// BOT3: the height-3 subtree under a depth n-3 node, fully in registers.
// Node numbering inside the subtree (posi): q0 = p0; q1,q2 = 2p0+1, 2p0+2;
// q3..q6 = 4p0+3 .. 4p0+6; leaves k0..k0+7 (k0 = 8*node).
// In-register lineage state per set: x[0] = W3 (8 symbols of q0) and x[1] =
// W2 (bits 0-15, 4 symbols of the current depth n-2 node) | W1 (bits 16-23,
// 2 symbols) | bL (bit 24, left leaf decision) | c2 (bits 25-26, left result
// at depth n-1) | c3 (bits 27-30, left result at depth n-2).
// QPD_BOT3_BYTEIDX: bot3_op holds W3 and W2 in interleaved order (element k in
// the high nibble of byte k, element k + half in the low one: lut_byte in
// qpd_fast_lookup.hpp), so byte k is the table index of the lookup one level
// down as it lies -- as W1's byte is the leaves' since QPD_LEAF_T.  W1, the
// partial sums and everything stored to rows keep their order; BOTX keeps the
// element order throughout (bx_spec reads symbols by nibble position).
// ---------------------------------------------------------------------------
// Leaf lookups (the depth n-1 node's f / g table, lut4) of the leaf pair whose
// symbols a, b are nibbles 4, 5 of x1 (and, for g, the left decision u bit 24):
// QPD_LEAF_T = 1 (qpd_mop.hpp) -- the host stores the depth n-1 tables
// transposed (entry u * 256 + b * 16 + a, pack_tables in qpd_plan.hpp), so the
// index is x1's bits 16..23 (..24) as they lie: one field extract instead of
// two extracts, a shift and an or per leaf.
__device__ __forceinline__ uint32_t leaf_idx(uint32_t x1) {
    if constexpr (QPD_LEAF_T) return __builtin_amdgcn_ubfe(x1, 16, 8);
    return (((x1 >> 16) & 15u) << 4) | ((x1 >> 20) & 15u);
}
__device__ __forceinline__ uint32_t leaf_idx_g(uint32_t x1) {  // with u = bit 24
    if constexpr (QPD_LEAF_T) return __builtin_amdgcn_ubfe(x1, 16, 9);
    return (((x1 >> 24) & 1u) << 8) | leaf_idx(x1);
}

__device__ __forceinline__ uint32_t f_pair(uint32_t T, uint32_t hi, uint32_t w2) {  // 2 symbols of f(W2)
    return lut_vec<2>(T, w2, w2 >> 8, hi);
}
__device__ __forceinline__ uint32_t g_pair(uint32_t T, uint32_t c2, uint32_t w2) {  // 2 symbols of g(W2, c2)
    return lut_vec<2>(T, w2, w2 >> 8, c2);
}

template <bool kList, int LM, bool SPEC, int NS, class Path>
__device__ __forceinline__ void bot_pair(Path (&st)[NS], uint32_t (&x)[NS][2], uint32_t Tf, int fo, uint32_t Tg,
                                         double V, int vo, int fr, int gl, int gbase, int L, int lane, int *sel, int sstride,
                                         uint32_t (&c)[NS]) {
    double dm[NS];
    uint32_t bl[NS], br[NS];
    bool moved[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        dm[s] = 0;
        if (kList || !(fr & 1)) dm[s] = shfld(V, vo + (int)lut4(Tf, leaf_idx(x[s][1]) + fo));
    }
#if QPD_SPEC_RIGHT  // (SPEC: SCL-LUT; the FastSCL unit measured slower with it)
    // The right leaf's quanta for the decision the left leaf takes when its
    // selection is the identity (its hard decision, or 0 if frozen), looked up
    // before the left fork's test resolves: the lookup latency leaves the
    // chain of the ~2/3 of forks that move nothing; a fork that moves paths
    // looks it up again from the surviving lineage's word.
    double sdm[NS];
    if constexpr (kList && LM == 8 && SPEC) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const uint32_t hb = (fr & 1) ? 0u : (uint32_t)(dm[s] < 0);  // H4: SCL family `< 0`
            sdm[s] = shfld(V, vo + 16 + (int)lut4(Tg, (hb << 8) | leaf_idx(x[s][1])));
        }
    }
#endif
    leaf_decide<kList, LM>(st, dm, fr & 1, gl, gbase, L, lane, sel, sstride, x, bl, moved);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        x[s][1] = (x[s][1] & ~(1u << 24)) | (bl[s] << 24);
#if QPD_SPEC_RIGHT
        if constexpr (kList && LM == 8 && SPEC) {
            dm[s] = sdm[s];
            if (moved[s]) dm[s] = shfld(V, vo + 16 + (int)lut4(Tg, leaf_idx_g(x[s][1])));
            continue;
        }
#endif
        if (kList || !(fr & 2)) dm[s] = shfld(V, vo + 16 + (int)lut4(Tg, leaf_idx_g(x[s][1])));
    }
    leaf_decide<kList, LM>(st, dm, fr & 2, gl, gbase, L, lane, sel, sstride, x, br, moved);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const uint32_t bl2 = (x[s][1] >> 24) & 1u;
        c[s] = (bl2 ^ br[s]) | (br[s] << 1);
    }
}

// The subtree runs in four stages -- A: q0 left + leaves 0, 1; B: q1 g +
// leaves 2, 3; C: q0 right + leaves 4, 5; D: q2 g + leaves 6, 7 -- and each
// stage issues the table / quanta loads of the next one (LAZY: SCL-LUT, with
// QPD_BOT3_LAZY; +0.5 % there at 5 waves, r04h), so at most about
// 11 of them are live at once: the register budget of a fifth wave per SIMD.
// `prefetch_next` issues the next op's operand prefetch at the start of stage
// D instead of at the start of this op (4 registers less through stages A-C).
// LT: the folded parent's lookups (MF_BFG) from its table staged as bytes at tb (lut_lds).
// LO (rows in lookup order, QPD_ROW_BYTEIDX): a row or pre-pass row of 8 symbols is W3 in
// interleaved order as it lies, the folded parent's 16 symbols two index words.
template <bool kList, int LM, bool LAZY, bool LT, bool CH, bool LO, int NS, class PF, class Path>
__device__ __forceinline__ void bot3_op(const FastPlan &P, const Mem (&M)[NS], const MOp &op,
                                        const int32_t *const (&y)[NS], Path (&st)[NS], uint32_t Tf0, uint32_t T2, int gl,
                                        int gbase, int L, int *sel, int sstride, int lane, PF &&prefetch_next,
                                        uint8_t *tb) {
    constexpr bool BI = QPD_BOT3_BYTEIDX != 0;
    static_assert(BI || !LO, "QPD_ROW_BYTEIDX needs QPD_BOT3_BYTEIDX: a row of 8 symbols is held as BOT3 holds W3");
    const int p0 = op.tab * QPD_EXP_TABMUL;
    const int fr = op.cnt;
    const uint32_t *ft = P.f_tab, *gt = P.g_tab;
    // Tables of the 7 internal nodes (q0's f table arrives prefetched).  Two
    // 32-dword f tables share one register (lanes 0-31 | 32-63: p and p+1 are
    // adjacent), addressed by adding 256 to the nibble index of the second.
    const int p1 = 2 * p0 + 1, p3 = 4 * p0 + 3;
    // Leaf quanta vcl[n-1][8*node + j][s] of the 8 leaves, four leaves per
    // register: lane 16*jj + s holds leaf 4*h + jj (v <= 16).
    const int v = P.v;
    const int s16 = lane & 15, j16 = lane >> 4;
    const double *vb = P.vcl + op.vrow * QPD_EXP_TABMUL;
    // stage A's operands, and B's
    const uint32_t Tf12 = tab_ld(ft, p1 * 32, lane);
    const uint32_t Tf34 = tab_ld(ft, p3 * 32, lane), Tg3 = tab_ld(gt, p3 * 64, lane);
    const double Vlo = s16 < v ? vb[j16 * v + s16] : 0.0;
    const uint32_t Tg1 = tab_ld(gt, p1 * 64, lane), Tg4 = tab_ld(gt, (p3 + 1) * 64, lane);
    uint32_t Tg0 = 0, Tf56 = 0, Tg5 = 0, Tg2 = 0, Tg6 = 0;
    double Vhi = 0.0;
    if constexpr (!LAZY) {
        Tg0 = tab_ld(gt, p0 * 64, lane);
        Tf56 = tab_ld(ft, (p3 + 2) * 32, lane);
        Tg5 = tab_ld(gt, (p3 + 2) * 64, lane);
        Tg2 = tab_ld(gt, (p1 + 1) * 64, lane);
        Tg6 = tab_ld(gt, (p3 + 3) * 64, lane);
        Vhi = s16 < v ? vb[(4 + j16) * v + s16] : 0.0;
    }
    uint32_t x[NS][2], c[NS];
    if (op.flags & MF_BFG) {
        // The depth n-4 parent's f / g (SCLLUTDecoder.cpp:83-89 / :157-164,
        // ctemp = 8) folded in: W3 from the parent's 16 symbols, in registers.
        const bool sl = op.flags & MF_SRC_LDS, ul = op.flags & MF_U_LDS;
        if constexpr (LT) stage_tab(tb, T2, (op.flags & MF_BG) ? gtab_dw(lane) : (lane & 31));
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int src = gbase + pfield(st[s].ps, op.sh_src);
            const uint32_t a = M[s].ld(sl, op.src_row, src), b = M[s].ld(sl, op.src_row + 1, src);
            const uint32_t ub = (op.flags & MF_BG) ? M[s].ld(ul, op.u_row, gbase + pfield(st[s].U(), op.sh_u)) : 0u;
            // (ub = 0 for f: entries < 256); the parent's lookup places W3's nibbles where BOT3 wants them
            if constexpr (LO) {  // (U[n-3]'s bits 0-3 / 4-7: the halves of a's / b's elements)
                x[s][0] = LT ? lut_lds<8, true, 0, true, true>(a, b, ub, ub >> 4) : lut_vec<8, true, true>(T2, a, b, ub, ub >> 4);
                continue;
            }
            x[s][0] = LT ? lut_lds<8, true, 0, BI>(a, b, ub) : lut_vec<8, BI>(T2, a, b, ub);
        }
    } else {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            x[s][0] = sym_word<CH>(P, M[s], op, y[s], gbase + pfield(st[s].ps, op.sh_src), 0);  // W3
            if constexpr (LO) {  // a row is in that order already; the channel (N = 8) is permuted once
                if (CH && (op.flags & MF_CHAN)) x[s][0] = nib_interleave8(x[s][0]);
                continue;
            }
            if constexpr (BI) x[s][0] = nib_interleave8(x[s][0]);  // from a row / the channel: permuted once
        }
    }
    // ---- q0 left: W2 = f(W3); q1: W1 = f(W2)
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        if constexpr (BI) {
            const uint32_t w2 = lut_byte<4, true, false>(Tf0, x[s][0]);
            x[s][1] = w2 | (lut_byte<2, false, false>(Tf12, w2) << 16);
            continue;
        }
        const uint32_t w2 = lut_vec<4>(Tf0, x[s][0], x[s][0] >> 16, 0u);
        x[s][1] = w2 | (f_pair(Tf12, 0u, w2) << 16);
    }
    bot_pair<kList, LM, LAZY>(st, x, Tf34, 0, Tg3, Vlo, 0, fr, gl, gbase, L, lane, sel, sstride, c);  // leaves 0, 1
    if constexpr (LAZY) {  // stage C's operands
        Tg0 = tab_ld(gt, p0 * 64, lane);
        Tf56 = tab_ld(ft, (p3 + 2) * 32, lane);
        Tg5 = tab_ld(gt, (p3 + 2) * 64, lane);
        Vhi = s16 < v ? vb[(4 + j16) * v + s16] : 0.0;
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {  // q1: W1 = g(W2, c2)
        x[s][1] = (x[s][1] & ~(3u << 25)) | (c[s] << 25);
        if constexpr (BI) {
            x[s][1] = (x[s][1] & ~(0xffu << 16)) | (lut_byte<2, false, true>(Tg1, x[s][1], half_bits2(c[s])) << 16);
            continue;
        }
        x[s][1] = (x[s][1] & ~(0xffu << 16)) | (g_pair(Tg1, c[s], x[s][1] & 0xffffu) << 16);
    }
    bot_pair<kList, LM, LAZY>(st, x, Tf34, 256, Tg4, Vlo, 32, fr >> 2, gl, gbase, L, lane, sel, sstride, c);  // leaves 2, 3
    if constexpr (LAZY) {  // stage D's operands
        Tg2 = tab_ld(gt, (p1 + 1) * 64, lane);
        Tg6 = tab_ld(gt, (p3 + 3) * 64, lane);
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const uint32_t c2 = (x[s][1] >> 25) & 3u;
        const uint32_t c3 = (c2 ^ c[s]) | (c[s] << 2);  // combine at depth n-2
        // ---- q0 right: W2 = g(W3, c3); q2: W1 = f(W2)
        if constexpr (BI) {
            const uint32_t w2 = lut_byte<4, true, true>(Tg0, x[s][0], half_bits4(c3));
            x[s][1] = w2 | (lut_byte<2, false, true>(Tf12, w2, 0x8080u) << 16) | (c3 << 27);  // (the second f table)
            continue;
        }
        const uint32_t w2 = lut_vec<4>(Tg0, x[s][0], x[s][0] >> 16, c3);
        x[s][1] = w2 | (f_pair(Tf12, 3u, w2) << 16) | (c3 << 27);
    }
    bot_pair<kList, LM, LAZY>(st, x, Tf56, 0, Tg5, Vhi, 0, fr >> 4, gl, gbase, L, lane, sel, sstride, c);  // leaves 4, 5
    if constexpr (LAZY) prefetch_next();
#pragma unroll
    for (int s = 0; s < NS; ++s) {  // q2: W1 = g(W2, c2)
        x[s][1] = (x[s][1] & ~(3u << 25)) | (c[s] << 25);
        if constexpr (BI) {
            x[s][1] = (x[s][1] & ~(0xffu << 16)) | (lut_byte<2, false, true>(Tg2, x[s][1], half_bits2(c[s])) << 16);
            continue;
        }
        x[s][1] = (x[s][1] & ~(0xffu << 16)) | (g_pair(Tg2, c[s], x[s][1] & 0xffffu) << 16);
    }
    bot_pair<kList, LM, LAZY>(st, x, Tf56, 256, Tg6, Vhi, 32, fr >> 6, gl, gbase, L, lane, sel, sstride, c);  // leaves 6, 7
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const uint32_t c2 = (x[s][1] >> 25) & 3u;
        const uint32_t c3r = (c2 ^ c[s]) | (c[s] << 2);
        const uint32_t c3l = (x[s][1] >> 27) & 15u;
        uint32_t res = (c3l ^ c3r) | (c3r << 4);  // combine at depth n-3
        if (op.flags & MF_BCOMB)  // and the parent's (utils.cpp:62-67): U[n-3] of this lineage ^ res | res
            res = ((M[s].ld(op.flags & MF_U_LDS, op.u_row, gbase + pfield(st[s].U(), op.sh_u)) & 0xFFu) ^ res) | (res << 8);
        if (op.flags & MF_BC2) {  // and the grandparent's: U[n-4] ^ res | res, 32 bits
            const int e = op.pad1;
            res = ((M[s].ld(op.flags & MF_BC2_ULDS, op.r_row, gbase + pfield(st[s].U(), e & 255)) & 0xFFFFu) ^ res) |
                  (res << 16);
            M[s].st(op.flags & MF_BC2_DLDS, e >> 16, lane, res);
            if (!(op.flags & MF_BC2_TOR)) st[s].U() = pset(st[s].U(), (e >> 8) & 255, gl);
            continue;
        }
        M[s].st(op.flags & MF_DST_LDS, op.dst_row, lane, res);
        if (!(op.flags & MF_TO_R)) st[s].U() = pset(st[s].U(), op.sh_dst, gl);
    }
}

// ---------------------------------------------------------------------------
// BOTX (FastSCL-LUT, L = 8; MF_BOTX): a height-3 subtree whose nodes of size
// 4 or 2 include FastSCL special nodes (FastSCLLUTDecoder.cpp:83-213: R0, R1,
// REP), held in registers like BOT3.  The types ride in op.cnt bits 8-19, two
// bits per node: q1, q2 (size 4), then q3..q6 (size 2); 0 = plain (a size-4
// node of two size-2 children / a leaf pair), else BX_R0 / BX_R1 / BX_REP
// (nodes inside a special one: don't care).  Every special node's elements
// share one quanta row (MF_VUNI's condition, checked by the host), which sits
// in lanes 0-15 of the slot's quanta register.  The subtree runs as four leaf
// slots (the pairs under q3..q6), a loop that is not unrolled, each slot
// loading its own tables and quanta: a size-4 special node takes its half's
// first slot and skips the second.  Special-node forks move the in-register lineage
// state x as the leaf forks do.
// ---------------------------------------------------------------------------
constexpr int BX_PLAIN = 0, BX_R0 = 1, BX_R1 = 2, BX_REP = 3;

// One special node of t = 2 or 4 elements for one frame set: its symbols are
// nibbles `base`/4.. of x[1], its quanta row q[sym] = lane sym of Vq.
// Returns the node's partial-sum bits (the codeword the reference writes to
// ucap: R0 zeros, REP all equal, R1 the hard decisions with the layers' flips).
template <class Path>
__device__ __forceinline__ uint32_t bx_spec(Path &st, uint32_t (&x)[2], int type, int t, int base, double Vq, int gl,
                                            int gbase, int L, int lane, int *sel, int sj) {
    double l[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) l[j] = shfld(Vq, (int)((x[1] >> (base + 4 * j)) & 15u));  // (j >= t: unused)
    if (type == BX_R0) {  // :83-98, (float)(l<0)·|l| as a select (H5: element order)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < t) st.pm += l[j] < 0 ? fabs(l[j]) : 0.0;
        return 0u;
    }
    if (type == BX_REP) {  // :169-213: the all-zeros / all-ones codewords as keep / flip
        double kk = st.pm, kf = st.pm;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < t) {
                kk += l[j] < 0 ? fabs(l[j]) : 0.0;
                kf += l[j] >= 0 ? fabs(l[j]) : 0.0;
            }
        if (keep_all8(__builtin_bit_cast(uint64_t, kk), __builtin_bit_cast(uint64_t, kf), gl)) {
            st.pm = kk;
            return 0u;
        }
        const Sel sx = select_survivors8(kk, kf, gl, gbase, lane, sel, sj);
        const int p = gbase + sx.parent;
        st.pm = pick(sx.upper, shfld(kf, p), shfld(kk, p));
        st.move(p);
        x[0] = (uint32_t)lane_read((int)x[0], p);
        x[1] = (uint32_t)lane_read((int)x[1], p);
        return sx.upper ? (1u << t) - 1u : 0u;
    }
    // R1 (:100-166): the stable argsort of |l| (std::sort of <= 16 elements is
    // an insertion sort, H1), packed with the lineage: r = ord (2 bits per rank)
    // | the ranked elements' symbols (4 bits each, from bit 8) | the decisions
    // (from bit 24, hard decisions l < 0, flipped per layer).  r follows the
    // survivors; a layer's flip position is the slot's own ord (H2).
    uint32_t r = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < t) {
            const double aj = fabs(l[j]);
            int rk = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < t && i != j) rk += (fabs(l[i]) < aj) || (fabs(l[i]) == aj && i < j);
            r |= ((uint32_t)j << (2 * rk)) | ((((x[1] >> (base + 4 * j)) & 15u)) << (8 + 4 * rk)) |
                 ((uint32_t)(l[j] < 0) << (24 + j));
        }
    }
    const int m = (L - 1) < t ? (L - 1) : t;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q < m) {
            const double ms = fabs(shfld(Vq, (int)((r >> (8 + 4 * q)) & 15u)));
            const double kf = st.pm + ms;
            // identity in every group: the later layers' flips are no smaller (ascending |l|)
            if (keep_all8(__builtin_bit_cast(uint64_t, st.pm), __builtin_bit_cast(uint64_t, kf), gl)) break;
            const Sel sx = select_survivors8(st.pm, kf, gl, gbase, lane, sel, sj);
            const int p = gbase + sx.parent;
            st.pm = pick(sx.upper, shfld(kf, p), shfld(st.pm, p));
            st.move(p);
            x[0] = (uint32_t)lane_read((int)x[0], p);
            x[1] = (uint32_t)lane_read((int)x[1], p);
            // H2: the flip position is this slot's own ord[q] before the move
            // (sorted_absllr_idx[i][layer], :136-140), the decisions the parent's
            const uint32_t own = (r >> (2 * q)) & 3u;
            r = (uint32_t)lane_read((int)r, p);
            if (sx.upper) r ^= 1u << (24 + own);
        }
    }
    return (r >> 24) & ((1u << t) - 1u);
}

// bx_spec for all the wave's frame sets at once: the sums interleaved element
// by element, the R1 layers of the sets interleaved (each set stops at its
// first identity layer) -- the sets' dependency chains overlap.
template <int NS, class Path>
__device__ __forceinline__ void bx_spec_multi(Path (&st)[NS], uint32_t (&x)[NS][2], int type, int t, int base, double Vq, int gl,
                                              int gbase, int lane, int *sel_all, int sstride, uint32_t (&res)[NS]) {
    auto fork = [&](int s, double keep, double flip, Sel &sx) {  // survivor exchange of set s (keep / flip keys)
        sx = select_survivors8(keep, flip, gl, gbase, lane, sel_all + sstride * s, NS * sstride);
        const int p = gbase + sx.parent;
        st[s].pm = pick(sx.upper, shfld(flip, p), shfld(keep, p));
        st[s].move(p);
        x[s][0] = (uint32_t)lane_read((int)x[s][0], p);
        x[s][1] = (uint32_t)lane_read((int)x[s][1], p);
        return p;
    };
#ifdef QPD_BXE
    if (QPD_BXE & 1) return;
#endif
    if (type != BX_R1) {  // R0 (:83-98) / REP (:169-213)
        double kk[NS], kf[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) kk[s] = kf[s] = st[s].pm;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < t)
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const double l = shfld(Vq, (int)((x[s][1] >> (base + 4 * j)) & 15u));
                    kk[s] += l < 0 ? fabs(l) : 0.0;  // H5: element order
                    if (type == BX_REP) kf[s] += l >= 0 ? fabs(l) : 0.0;
                }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            res[s] = 0u;
            if (type == BX_R0 || keep_all8(__builtin_bit_cast(uint64_t, kk[s]), __builtin_bit_cast(uint64_t, kf[s]), gl)) {
                st[s].pm = kk[s];
            } else {
                Sel sx;
                fork(s, kk[s], kf[s], sx);
                res[s] = sx.upper ? (1u << t) - 1u : 0u;
            }
        }
        return;
    }
#ifdef QPD_BXE
    if (QPD_BXE & 2) return;
#endif
    // R1 (:100-166): per set r = ord | ranked symbols | decisions, as bx_spec
    uint32_t r[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        double a[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = shfld(Vq, (int)((x[s][1] >> (base + 4 * j)) & 15u));
        r[s] = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < t) {
                const double aj = fabs(a[j]);
                int rk = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < t && i != j) rk += (fabs(a[i]) < aj) || (fabs(a[i]) == aj && i < j);
                r[s] |= ((uint32_t)j << (2 * rk)) | (((x[s][1] >> (base + 4 * j)) & 15u) << (8 + 4 * rk)) |
                        ((uint32_t)(a[j] < 0) << (24 + j));
            }
        }
    }
    bool done[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) done[s] = false;
#pragma unroll 1
    for (int q = 0; q < t; ++q) {  // m = min(L - 1, t) = t (L = 8, t <= 4)
        double kf[NS];
        bool all = true;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (done[s]) continue;
            kf[s] = st[s].pm + fabs(shfld(Vq, (int)((r[s] >> (8 + 4 * q)) & 15u)));
            done[s] = keep_all8(__builtin_bit_cast(uint64_t, st[s].pm), __builtin_bit_cast(uint64_t, kf[s]), gl);
            all = all && done[s];
        }
        if (all) break;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (done[s]) continue;
            Sel sx;
            const int p = fork(s, st[s].pm, kf[s], sx);
            const uint32_t own = (r[s] >> (2 * q)) & 3u;  // H2: this slot's own ord[q]
            r[s] = (uint32_t)lane_read((int)r[s], p);
            if (sx.upper) r[s] ^= 1u << (24 + own);
        }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) res[s] = (r[s] >> 24) & ((1u << t) - 1u);
}

// Operands of one leaf slot k (the pair under q3 + k): the table the half's W2
// comes from (k even: q0's f for k = 0, g for k = 2), the size-4 node's f (k
// even) or g table, the pair node's f and g tables, and the quanta register
// (lanes 0-15: the size-4 special node's row, the size-2 special node's row,
// or the left leaf's row; lanes 16-31: the right leaf's row).
struct BxSlot {
    uint32_t t2, t1, tf, tg;
    double V;
};

__device__ __forceinline__ BxSlot bx_load(const FastPlan &P, const MOp &op, int k, int ty, int lane) {
    const int p0 = op.tab, p1 = 2 * p0 + 1, p3 = 4 * p0 + 3;
    const int h = k >> 1, sub = k & 1;
    const int t4 = (ty >> (2 * h)) & 3, t2 = (ty >> (4 + 2 * k)) & 3;
    BxSlot s;
    s.t2 = 0u;
    if (!sub) s.t2 = h ? tab_ld(P.g_tab, p0 * 64, lane) : tab_ld(P.f_tab, p0 * 32, lane & 31);
    s.t1 = sub ? tab_ld(P.g_tab, (p1 + h) * 64, lane) : tab_ld(P.f_tab, (p1 + h) * 32, lane & 31);
    s.tf = tab_ld(P.f_tab, (p3 + k) * 32, lane & 31);
    s.tg = tab_ld(P.g_tab, (p3 + k) * 64, lane);
    // quanta rows vcl[row][pos][sym]: node8 = op.node (the subtree root at depth n-3)
    const int n = P.n, N = P.N, v = P.v, sym = lane & 15, j = (lane >> 4) & 1;
    const int pos8 = 8 * op.node;
    int row = n - 1, pos = pos8 + 2 * k + j;  // leaf rows
    if (t4 != BX_PLAIN) row = n - 3, pos = pos8 + 4 * h;  // size-4 special node (row d - 1, H3)
    else if (t2 != BX_PLAIN) row = n - 2, pos = pos8 + 2 * k;
    s.V = sym < v ? P.vcl[((size_t)row * N + pos) * v + sym] : 0.0;
    return s;
}

template <bool LT, bool CH, int NS, class Path>
__device__ __forceinline__ void botx_op(const FastPlan &P, const Mem (&M)[NS], const MOp &op, const int32_t *const (&y)[NS],
                                        Path (&st)[NS], uint32_t Tf0, uint32_t T2, int gl, int gbase, int L, int *sel,
                                        int sstride, int lane, uint8_t *tb) {
    const int fr = op.cnt & 0xff, ty = (op.cnt >> 8) & 0xfff;
    uint32_t x[NS][2], c[NS], c3r[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) x[s][1] = c3r[s] = 0u;
#if QPD_BX_PIPE
    BxSlot nx = bx_load(P, op, 0, ty, lane);
#endif
    if (op.flags & MF_BFG) {  // the depth n-4 parent's f / g folded in (as bot3_op)
        const bool sl = op.flags & MF_SRC_LDS, ul = op.flags & MF_U_LDS;
        if constexpr (LT) stage_tab(tb, T2, (op.flags & MF_BG) ? gtab_dw(lane) : (lane & 31));
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int src = gbase + pfield(st[s].ps, op.sh_src);
            const uint32_t a = M[s].ld(sl, op.src_row, src), b = M[s].ld(sl, op.src_row + 1, src);
            const uint32_t ub = (op.flags & MF_BG) ? M[s].ld(ul, op.u_row, gbase + pfield(st[s].U(), op.sh_u)) : 0u;
            x[s][0] = LT ? lut_lds<8, true>(a, b, ub) : lut_vec<8>(T2, a, b, ub);
        }
    } else {
#pragma unroll
        for (int s = 0; s < NS; ++s) x[s][0] = sym_word<CH>(P, M[s], op, y[s], gbase + pfield(st[s].ps, op.sh_src), 0);
    }
    (void)Tf0;
#pragma unroll 1  // (unrolled: 18 % slower)
    for (int k = 0; k < 4; ++k) {
        const int h = k >> 1, sub = k & 1;
        const int t4 = (ty >> (2 * h)) & 3, t2 = (ty >> (4 + 2 * k)) & 3;
        if (t4 != BX_PLAIN && sub) continue;  // the half's size-4 special node ran at slot k - 1
#if QPD_BX_PIPE
        const BxSlot cur = nx;
        const int kn = t4 != BX_PLAIN ? k + 2 : k + 1;  // the next slot run
        if (kn < 4) nx = bx_load(P, op, kn, ty, lane);
#else
        const BxSlot cur = bx_load(P, op, k, ty, lane);
#endif
        if (!sub) {
#pragma unroll
            for (int s = 0; s < NS; ++s) {  // W2 = f(W3) / g(W3, c3) (q0, SCLLUTDecoder.cpp:83-89 / :157-164)
                const uint32_t w2 = lut_vec<4>(cur.t2, x[s][0], x[s][0] >> 16, h ? (x[s][1] >> 27) & 15u : 0u);
                x[s][1] = (x[s][1] & (15u << 27)) | w2;
            }
        }
        if (t4 != BX_PLAIN) {  // q1 / q2 special
            uint32_t res[NS];
            bx_spec_multi(st, x, t4, 4, 0, cur.V, gl, gbase, lane, sel, sstride, res);
#pragma unroll
            for (int s = 0; s < NS; ++s) {
                if (h) c3r[s] = res[s];
                else x[s][1] = (x[s][1] & ~(15u << 27)) | (res[s] << 27);
            }
            continue;
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {  // W1 = f(W2) / g(W2, c2) (q1 / q2)
            const uint32_t w2 = x[s][1] & 0xffffu;
            const uint32_t w1 = sub ? g_pair(cur.t1, (x[s][1] >> 25) & 3u, w2) : f_pair(cur.t1, 0u, w2);
            x[s][1] = (x[s][1] & ~(0xffu << 16)) | (w1 << 16);
        }
#ifdef QPD_BXE
        if (QPD_BXE & 4) continue;
#endif
        if (t2 == BX_PLAIN) {
            bot_pair<true, 8, false>(st, x, cur.tf, 0, cur.tg, cur.V, 0, fr >> (2 * k), gl, gbase, L, lane, sel, sstride, c);
        } else {
            bx_spec_multi(st, x, t2, 2, 16, cur.V, gl, gbase, lane, sel, sstride, c);
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (!sub) {
                x[s][1] = (x[s][1] & ~(3u << 25)) | (c[s] << 25);
            } else {
                const uint32_t c2 = (x[s][1] >> 25) & 3u;
                const uint32_t c3 = (c2 ^ c[s]) | (c[s] << 2);  // combine at depth n-2
                if (h) c3r[s] = c3;
                else x[s][1] = (x[s][1] & ~(15u << 27)) | (c3 << 27);
            }
        }
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {  // as the end of bot3_op
        const uint32_t c3l = (x[s][1] >> 27) & 15u;
        uint32_t res = (c3l ^ c3r[s]) | (c3r[s] << 4);  // combine at depth n-3
        if (op.flags & MF_BCOMB)
            res = ((M[s].ld(op.flags & MF_U_LDS, op.u_row, gbase + pfield(st[s].U(), op.sh_u)) & 0xFFu) ^ res) | (res << 8);
        if (op.flags & MF_BC2) {
            const int e = op.pad1;
            res = ((M[s].ld(op.flags & MF_BC2_ULDS, op.r_row, gbase + pfield(st[s].U(), e & 255)) & 0xFFFFu) ^ res) |
                  (res << 16);
            M[s].st(op.flags & MF_BC2_DLDS, e >> 16, lane, res);
            if (!(op.flags & MF_BC2_TOR)) st[s].U() = pset(st[s].U(), (e >> 8) & 255, gl);
            continue;
        }
        M[s].st(op.flags & MF_DST_LDS, op.dst_row, lane, res);
        if (!(op.flags & MF_TO_R)) st[s].U() = pset(st[s].U(), op.sh_dst, gl);
    }
}

}  // namespace qpd
