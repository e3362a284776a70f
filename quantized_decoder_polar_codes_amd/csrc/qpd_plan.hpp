// qpd_plan.hpp -- the fast engine's plan compiler (host code, no HIP): from a
// code and its traversal schedule to everything the kernels of qpd_fast.hip
// read -- per-depth placement of the path buffers (deep levels in LDS, shallow
// levels in a global slab, sized to the LDS budget per wave), nibble-packed
// per-node tables, and the micro-op lists with every offset precomputed and
// plain height-3 subtrees fused into BOT3 ops.  plan_fast() is the entry
// point; qpd_capi.hip (build_fast) puts its result on the device, and
// tests/test_plan.py checks it on the CPU.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "qpd.h"
#include "qpd_mop.hpp"
#include "qpd_schedule.hpp"
#include "stl_sort.hpp"

namespace qpd_plan {

using qpd_sched::Schedule;
using qpd_sched::special_of;

// Every switch of the plan compiler, read from the environment once per
// qpd_create (from_env).  This is the one description of each switch; all are
// for measurements and tests, the defaults are the product.  The QPD_NO_*
// variables are on when set to any value, even an empty one.
struct PlanSwitches {
    static constexpr int kUnset = INT_MIN;
    int sets = 0;                // QPD_SETS: frame sets per wave, 1 or 2 (0: the kind's default); a -DQPD_SETS3
                                 //   build also admits 3, for SCL-LUT with L = 8
    int lds_budget = kUnset;     // QPD_LDS_BUDGET: LDS bytes per wave the layout may use (kUnset: by the sets)
    int64_t pre_chunk = 0;       // QPD_PRE_CHUNK: frames per pre-pass chunk, >= 1 (0: 8 GB of rows)
    int pfx_sets = 0;            // QPD_PFX_SETS: frame sets of the prefix stages, >= 1 and at most min(sets, 2) (0: that)
    bool pfx1b = false;          // QPD_PFX1B: prefix stage 1b (two live paths) between stages 1 and 2
    bool no_pre = false;         // QPD_NO_PRE: no root pre-pass (MF_PRE / MF_GSEL); with it go the prefix stages
    bool no_bfuse = false;       // QPD_NO_BFUSE: depth n-4 nodes keep their F / G / COMB ops (no MF_BFG / MF_BCOMB)
    bool no_botx = false;        // QPD_NO_BOTX: no mixed bottom subtrees and no folded special nodes (MF_BOTX, MF_SFG)
    bool no_trim = false;        // QPD_NO_TRIM: the layout keeps the row slots no op touches
    bool no_pfx = false;         // QPD_NO_PFX: no frozen-prefix stages
    bool no_pfx2 = false;        // QPD_NO_PFX2: no prefix stage 2 (four live paths)
    bool no_ff = false;          // QPD_NO_FF: no folded descents (MF_FF, fuse_descent)
    bool no_bc2 = false;         // QPD_NO_BC2: no folded depth n-5 combines (MF_BC2, fold_combine)
    bool no_pw1 = false;         // QPD_NO_PW1: two pointer words per path (no compact_pointer_fields)
    bool no_vuni = false;        // QPD_NO_VUNI: special nodes gather their quanta per element (no MF_VUNI)
    bool no_r1rk = false;        // QPD_NO_R1RK: R1 nodes look their ranks up in the rank table (no MF_R1_RK)
    bool no_sfold = false;       // QPD_NO_SFOLD: size-8 special nodes keep their parent's F / G / COMB ops
#ifdef QPD_DIAG
    int botx_sel = -1;           // QPD_BOTX_SEL: special nodes a mixed bottom subtree may hold -- allowed types
                                 //   (bit 1 R0, 2 R1, 3 REP) | sizes (bit 4: 4, bit 5: 2)
#endif
    static PlanSwitches from_env() {
        PlanSwitches w;
        auto on = [](const char *name) { return getenv(name) != nullptr; };
        if (const char *e = getenv("QPD_SETS")) {
            w.sets = std::min(2, std::max(1, atoi(e)));
#ifdef QPD_SETS3
            if (atoi(e) == 3) w.sets = 3;
#endif
        }
        if (const char *e = getenv("QPD_LDS_BUDGET")) w.lds_budget = atoi(e);
        if (const char *e = getenv("QPD_PRE_CHUNK")) w.pre_chunk = std::max<int64_t>(1, atoll(e));
        if (const char *e = getenv("QPD_PFX_SETS")) w.pfx_sets = std::max(1, atoi(e));
        w.pfx1b = on("QPD_PFX1B");
        w.no_pre = on("QPD_NO_PRE");
        w.no_bfuse = on("QPD_NO_BFUSE");
        w.no_botx = on("QPD_NO_BOTX");
        w.no_trim = on("QPD_NO_TRIM");
        w.no_pfx = on("QPD_NO_PFX");
        w.no_pfx2 = on("QPD_NO_PFX2");
        w.no_ff = on("QPD_NO_FF");
        w.no_bc2 = on("QPD_NO_BC2");
        w.no_pw1 = on("QPD_NO_PW1");
        w.no_vuni = on("QPD_NO_VUNI");
        w.no_r1rk = on("QPD_NO_R1RK");
        w.no_sfold = on("QPD_NO_SFOLD");
#ifdef QPD_DIAG
        if (const char *e = getenv("QPD_BOTX_SEL")) w.botx_sel = atoi(e);
#endif
        return w;
    }
};

struct FastLayout {
    int D = 0;
    int S[qpd::kMaxDepth + 1] = {}, U[qpd::kMaxDepth + 1] = {}, R[qpd::kMaxDepth + 1] = {};
    // LDS rows are grouped by depth (R, S, U of depth D, then of D+1, ...) and
    // followed by the set's selection scratch, so that the rows of all depths
    // > d form one contiguous tail: free scratch while a special node at
    // depth d (which replaces its whole subtree) runs.
    int lds_base[qpd::kMaxDepth + 2] = {};  // first LDS row of depth dd (dd >= D)
    int lds_end = 0;                        // rows incl. the selection scratch
    bool pre = false;    // root pre-pass (root_pre_kernel): MF_PRE / MF_GSEL ops at the root
    bool bfuse = false;  // BOT3 children of depth n-4 nodes fold in the parent's F / G / COMB
    int ns = 1;          // frame sets per wave (their rows interleave)
    bool botx = false;   // FastSCL-LUT, L = 8: height-3 subtrees with special nodes as BOT3 ops (MF_BOTX)
    bool lds(int dd) const { return dd >= D; }
};

// What plan_fast computes: everything of a fast plan that needs no device.
struct FastHostPlan {
    std::vector<qpd::MOp> ops;     // the decode kernel's list
    std::vector<qpd::MOp> pfx[3];  // frozen-prefix stages 1, 1b, 2 (plan_prefix); empty: no such stage
    int pfx_rec[3] = {}, pfx_pm[3] = {};  // per stage: words per (path) record, metric word in it
    std::vector<uint16_t> r1tab;   // FastSCL R1 rank keys (r1_rank_table), per node at op.tab
    std::vector<uint32_t> ft, gt;  // nibble-packed f / g tables (pack_tables)
    int lds_from = 0, lds_rows = 0, glb_rows = 0;
    int R0_row = 0, R0_lds = 0;              // root partial sums (R[0])
    int H_row = 0, K_row = 0, I_row = 0;     // R1 scratch (slab)
    int lds_bytes = 0, lds_tab_bytes = 0;    // LDS per wave; of it, the f / g ops' byte tables
    int lds_budget = 0;                      // the budget the layout was sized to
    int sets = 1, pfx_sets = 1;  // frame sets per wave: decode kernel, prefix stages
    bool l8 = false;   // list decoder with L = 8 (select_survivors8)
    bool w16 = false;  // SCL-LUT / FastSCL-LUT with 9 <= L <= 16 (lane groups of 16, select_survivors16)
    bool r1l = false;  // an R1 node needs r1_large (the R1L instantiation)
    bool pw1 = false;  // one pointer word per path (compact_pointer_fields)
    bool pre = false;  // root pre-pass
    bool row_lo = false;  // S rows of >= 8 symbols and the pre-pass rows in lookup order (QPD_ROW_BYTEIDX; MF_LO)
    int64_t pre_chunk = 0;  // frames per pre-pass chunk
    FastLayout layout;                  // the final layout and the row slots it keeps
    bool use[3][qpd::kMaxDepth + 1];    //   (slot 0 R, 1 S, 2 U; per depth): see make_owner
};

// A plain height-3 subtree under (d = n-3, node): one BOT3 op.
inline bool bot3_plain(int kind, const int32_t *node_type, int n, int d, int node) {
    if (n < 3 || d != n - 3) return false;
    for (int dd = d; dd < n; ++dd)
        for (int k = 0; k < (1 << (dd - d)); ++k)
            if (special_of(kind, node_type, (1 << dd) + (node << (dd - d)) + k - 1) >= 0) return false;
    return true;
}

// The elements of the special node (d, node) share one quanta row vcl[d-1][pos]
// (MF_VUNI's condition; every MinDistortion table qualifies).
inline bool quanta_uniform(const double *vcl, int N, int v, int d, int node) {
    const int temp = N >> d;
    const uint64_t *q = (const uint64_t *)(vcl + ((size_t)(d - 1) * N + (size_t)temp * node) * v);
    for (int j = 1; j < temp; ++j)
        if (std::memcmp(q, q + (size_t)j * v, sizeof(double) * v) != 0) return false;
    return true;
}

// A height-3 subtree under (d = n-3, node) that botx_op (qpd_fast_bot.hpp) can run in
// registers: its nodes of size 4 and 2 plain or FastSCL special nodes (R0 / R1 /
// REP) with one quanta row each.  *ty = the types, two bits per node (q1, q2,
// then q3..q6; BX_* in qpd_fast_bot.hpp).
inline bool bot3_mixed(const PlanSwitches &sw, int kind, const int32_t *node_type, const double *vcl, int N, int n, int v, int node,
                       int *ty) {
    if (kind != QPD_FASTSCL_LUT || n < 4 || v > 16) return false;
    const int d = n - 3;
    if (special_of(kind, node_type, (1 << d) + node - 1) >= 0) return false;
    int t = 0;
    bool any = false;
    for (int h = 0; h < 2; ++h) {
        const int q = 2 * node + h;  // size-4 node at depth n-2
        const int s4 = special_of(kind, node_type, (1 << (d + 1)) + q - 1);
        if (s4 >= 0) {
            if (!quanta_uniform(vcl, N, v, d + 1, q)) return false;
            t |= (1 + s4) << (2 * h);  // R0 / R1 / REP = 0 / 1 / 2 -> BX_R0 / BX_R1 / BX_REP
            any = true;
            continue;
        }
        for (int c = 0; c < 2; ++c) {
            const int k = 2 * h + c, q2 = 2 * q + c;  // size-2 node at depth n-1
            const int s2 = special_of(kind, node_type, (1 << (d + 2)) + q2 - 1);
            if (s2 < 0) continue;
            if (!quanta_uniform(vcl, N, v, d + 2, q2)) return false;
            t |= (1 + s2) << (4 + 2 * k);
            any = true;
        }
    }
#ifdef QPD_DIAG  // diagnostic builds only (PlanSwitches::botx_sel)
    for (int i = 0; i < 6; ++i) {
        const int x = (t >> (2 * i)) & 3;
        if (x && (!(sw.botx_sel & (1 << x)) || !(sw.botx_sel & (i < 2 ? 16 : 32)))) return false;
    }
#else
    (void)sw;
#endif
    *ty = t;
    return any;
}

// R1 argsort keys of the fast engine (FastSCL, node size <= 32): for element j
// and symbol s of the node, (rank of |vcl[d-1][pos_j][s]| among all the node's
// magnitudes) << 1 | (vcl < 0).  Equal magnitudes get equal ranks, so
// comparing ranks is comparing the doubles (H1 tie behaviour intact).
inline void r1_rank_table(std::vector<uint16_t> &tab, const double *vcl, int N, int v, int d, int node) {
    const int temp = N >> d;
    const double *q = vcl + ((size_t)(d - 1) * N + (size_t)temp * node) * v;
    std::vector<double> mags;
    for (int i = 0; i < temp * v; ++i) mags.push_back(std::fabs(q[i]));
    std::sort(mags.begin(), mags.end());
    mags.erase(std::unique(mags.begin(), mags.end()), mags.end());
    for (int i = 0; i < temp * v; ++i) {
        const int r = (int)(std::lower_bound(mags.begin(), mags.end(), std::fabs(q[i])) - mags.begin());
        tab.push_back((uint16_t)((r << 1) | (q[i] < 0 ? 1 : 0)));
    }
}

// The U-row pointer field of depth dd (1 .. n): nibble dd of the path's U word, and for dd = 16 (the
// leaf level of N = 65536) nibble 0, which no other U row uses -- the root's result goes to R[0]
// (MF_TO_R: no pointer) and no op reads U[0].  4 * 16 would be a shift by the word's whole width.
inline int u_field(int dd) { return 4 * (dd & 15); }

inline void fast_ops(std::vector<qpd::MOp> &out, const FastLayout &Ly, const PlanSwitches &sw, int kind, int N, int n, int v,
                     const int32_t *frozen, const int32_t *node_type, const double *vcl, std::vector<uint16_t> &r1tab, int d,
                     int node) {
    using namespace qpd;
    const int posi = (1 << d) + node - 1;
    auto base = [&](int type) {
        MOp m;
        std::memset(&m, 0, sizeof(m));
        m.type = type;
        m.d = d;
        m.node = node;
        m.sh_src = 4 * d;
        if (d == 0)
            m.flags |= MF_CHAN;
        else if (Ly.pre && d == 1 && node == 0)
            m.flags |= MF_PRE;  // f(y) words at the start of the frame's pre-pass row (src_row 0)
        else {
            m.src_row = Ly.S[d];
            if (Ly.lds(d)) m.flags |= MF_SRC_LDS;
        }
        return m;
    };
    auto finish_node = [&](MOp &m) {  // destination of a finished node (d, node)
        const bool to_r = d == 0 || (node & 1);
        m.dst_row = to_r ? Ly.R[d] : Ly.U[d];
        if (to_r) m.flags |= MF_TO_R;
        if (Ly.lds(d)) m.flags |= MF_DST_LDS;
        m.sh_dst = 4 * d;
    };
    const int t = special_of(kind, node_type, posi);
    if (t >= 0) {
        MOp m = base(OP_R0 + t);
        m.cnt = N >> d;
        m.vrow = (d - 1) * N + (N >> d) * node;
        if (v <= 16 && !sw.no_vuni) {  // one quanta row for all the node's elements (MinDistortion tables)
            const uint64_t *q = (const uint64_t *)(vcl + (size_t)m.vrow * v);
            bool uni = true;
            for (int j = 1; j < m.cnt && uni; ++j) uni = std::memcmp(q, q + (size_t)j * v, sizeof(double) * v) == 0;
            if (uni) m.flags |= MF_VUNI;
        }
        if (kind == QPD_FASTSCL_LUT && OP_R0 + t == OP_R1 && m.cnt <= 32) {
            m.tab = (int)r1tab.size();  // rank-key table of this node
            r1_rank_table(r1tab, vcl, N, v, d, node);
            if ((m.flags & MF_VUNI) && !sw.no_r1rk) {  // one row: the symbols' ranks (< 16) and signs in the record
                uint64_t rk = 0;
                uint32_t sg = 0;
                for (int sy = 0; sy < v; ++sy) {
                    const uint16_t e = r1tab[m.tab + sy];  // element 0's entry = every element's
                    rk |= (uint64_t)(e >> 1) << (4 * sy);
                    sg |= (uint32_t)(e & 1) << sy;
                }
                m.flags |= MF_R1_RK;
                m.r_row = (int32_t)(uint32_t)rk;
                m.tab2 = (int32_t)(uint32_t)(rk >> 32);
                m.pad1 = (int32_t)sg;
            }
            // > 16 elements: std::sort's introsort runs on 16-bit entries in the
            // free LDS tail of the wave (the sets' rows of depths > d + their
            // selection scratch; plan_fast pads the LDS rows to make room)
            if (m.cnt > qpd::stl::kThreshold && Ly.lds(d + 1) && Ly.ns * (Ly.lds_end - Ly.lds_base[d + 1]) >= m.cnt / 2) {
                m.flags |= MF_R1_LDS;
                m.u_row = Ly.lds_base[d + 1];
            }
        }
        finish_node(m);
        out.push_back(m);
        return;
    }
    int bx_ty = 0;
    if (n >= 3 && d == n - 3) {
        const bool mixed = Ly.botx && bot3_mixed(sw, kind, node_type, vcl, N, n, v, node, &bx_ty);
        if (mixed || bot3_plain(kind, node_type, n, d, node)) {
            MOp m = base(OP_BOT3);
            for (int j = 0; j < 8; ++j) m.cnt |= (frozen[8 * node + j] == 1) << j;
            if (mixed) {
                m.flags |= MF_BOTX;
                m.cnt |= bx_ty << 8;
            }
            m.tab = posi;
            m.vrow = ((n - 1) * N + 8 * node) * v;
            finish_node(m);
            out.push_back(m);
            return;
        }
    }
    if (d + 1 < n) {
        // Both children plain BOT3 subtrees of a depth n-4 node (d >= 2: S[d] is
        // a slab/LDS row): the left BOT3 takes this node's f, the right one its g
        // and then this node's combine -- no F / G / COMB ops, no S[n-3] rows.
        int t0 = 0;
        auto bot3_able = [&](int c) {  // the child (d + 1, c) becomes a BOT3 op
            return bot3_plain(kind, node_type, n, d + 1, c) ||
                   (Ly.botx && bot3_mixed(sw, kind, node_type, vcl, N, n, v, c, &t0));
        };
        // FastSCL-LUT (L = 8): a size-8 special child takes this node's f / g and combine too
        // (MF_SFG / MF_SGG / MF_SCOMB: r0rep_multi, r1_multi in qpd_fast_special.hpp); R1 only with its
        // ranks in the op record (MF_R1_RK: the record's tab field then holds this node's table)
        auto spec8_able = [&](int c) {
            const int cp = (1 << (d + 1)) + c - 1, ts = special_of(kind, node_type, cp);
            if (!Ly.botx || ts < 0 || sw.no_sfold) return false;
            return OP_R0 + ts != OP_R1 ||
                   (v <= 16 && quanta_uniform(vcl, N, v, d + 1, c) && !sw.no_vuni && !sw.no_r1rk);
        };
        const bool fuse = Ly.bfuse && d == n - 4 && d >= 2 && (bot3_able(2 * node) || spec8_able(2 * node)) &&
                          (bot3_able(2 * node + 1) || spec8_able(2 * node + 1));
        auto spec_child = [&](int c) { return !bot3_able(c); };  // (under `fuse`: a size-8 special child)
        for (int side = 0; side < 2; ++side) {
            MOp m = base(side ? OP_G : OP_F);
            m.cnt = N >> (d + 1);
            m.dst_row = Ly.S[d + 1];
            if (Ly.lds(d + 1)) m.flags |= MF_DST_LDS;
            m.sh_dst = 4 * (d + 1);
            if (side) {
                m.u_row = Ly.U[d + 1];
                if (Ly.lds(d + 1)) m.flags |= MF_U_LDS;
                m.sh_u = 4 * (d + 1);
                m.tab = posi * 64;
            } else {
                m.tab = posi * 32;
            }
            if (Ly.pre && d == 0) {  // root in pre-mode: f(y) comes from the pre-pass row, g(y, u) by selects
                m.flags = (m.flags & ~MF_CHAN) | MF_PRE | MF_GSEL;
                m.src_row = N >> 4;  // g(y, 0) words; g(y, 1) follow
            }
            if (fuse && spec_child(2 * node + side)) {
                const size_t at = out.size();
                fast_ops(out, Ly, sw, kind, N, n, v, frozen, node_type, vcl, r1tab, d + 1, 2 * node + side);
                MOp &b = out[at];  // the child's special op: this node's f / g (and combine) folded in
                b.flags = (b.flags & ~MF_SRC_LDS) | (m.flags & MF_SRC_LDS) | MF_SFG;
                b.src_row = m.src_row;
                b.sh_src = m.sh_src;
                b.tab = m.tab;
                if (side) {
                    b.flags = (b.flags & ~(MF_DST_LDS | MF_TO_R)) | MF_SGG | MF_SCOMB | (m.flags & MF_U_LDS);
                    b.u_row = m.u_row;  // U[n-3] of the left child: g's u bits, then the combine's left half
                    b.sh_u = m.sh_u;
                    finish_node(b);  // this node's destination
                }
                continue;
            }
            if (fuse) {
                const size_t at = out.size();
                fast_ops(out, Ly, sw, kind, N, n, v, frozen, node_type, vcl, r1tab, d + 1, 2 * node + side);
                MOp &b = out[at];  // the child's BOT3
                b.flags = (b.flags & ~MF_SRC_LDS) | (m.flags & MF_SRC_LDS) | MF_BFG;
                b.src_row = m.src_row;
                b.sh_src = m.sh_src;
                b.tab2 = m.tab;
                if (side) {
                    b.flags = (b.flags & ~(MF_DST_LDS | MF_TO_R)) | MF_BG | MF_BCOMB | (m.flags & MF_U_LDS);
                    b.u_row = m.u_row;  // U[n-3]: g's u bits, then the left half of the combine
                    b.sh_u = m.sh_u;
                    finish_node(b);  // this node's destination
                }
                continue;
            }
            if (!(Ly.pre && d == 0 && side == 0)) out.push_back(m);
            fast_ops(out, Ly, sw, kind, N, n, v, frozen, node_type, vcl, r1tab, d + 1, 2 * node + side);
        }
        if (fuse) return;
    } else {
        for (int side = 0; side < 2; ++side) {
            const int k = 2 * node + side;
            MOp m = base(side ? OP_LEAF_R : OP_LEAF_L);
            m.cnt = frozen[k] == 1;
            m.dst_row = side ? Ly.R[n] : Ly.U[n];
            if (Ly.lds(n)) m.flags |= MF_DST_LDS;
            m.sh_dst = u_field(n);
            if (side) {
                m.u_row = Ly.U[n];
                if (Ly.lds(n)) m.flags |= MF_U_LDS;
                m.sh_u = u_field(n);
                m.tab = posi * 64;
            } else {
                m.tab = posi * 32;
            }
            m.vrow = ((n - 1) * N + k) * v;
            out.push_back(m);
        }
    }
    MOp m = base(OP_COMB);
    m.cnt = N >> (d + 1);
    m.u_row = Ly.U[d + 1];
    m.r_row = Ly.R[d + 1];
    if (Ly.lds(d + 1)) m.flags |= MF_U_LDS | MF_R_LDS;
    m.sh_u = u_field(d + 1);
    finish_node(m);
    out.push_back(m);
}

// Fold an F at depth d+1 into the F / G right before it that produced its
// input (MF_FF, ff_op in qpd_fast_lookup.hpp): the child's f reads the words the
// parent just computed from registers instead of re-reading S[d+1] from the
// slab.  Pairs are taken greedily down each descent (G1+F2, F3+F4, ...);
// S[d] and S[d+1] as the slab rows ff_op reads, S[d+1] of at least 4 words.
// The rows written are the same as before, so the prefix split's analysis
// (op_rows on the unfused list) and the stores' order are unchanged.
inline void fuse_descent(std::vector<qpd::MOp> &ops) {
    using namespace qpd;
    std::vector<MOp> out;
    out.reserve(ops.size());
    for (size_t i = 0; i < ops.size(); ++i) {
        MOp a = ops[i];
        if (i + 1 < ops.size() && (a.type == OP_F || a.type == OP_G) &&
            !(a.flags & (MF_CHAN | MF_PRE | MF_GSEL | MF_SRC_LDS | MF_FF)) && a.cnt >= 32) {
            const MOp &b = ops[i + 1];
            const bool dl = a.flags & MF_DST_LDS, cdl = b.flags & MF_DST_LDS;
            if (b.type == OP_F && b.d == a.d + 1 && b.src_row == a.dst_row && b.sh_src == a.sh_dst &&
                ((b.flags & MF_SRC_LDS) != 0) == dl && !(dl && !cdl) && !(b.flags & (MF_CHAN | MF_PRE | MF_GSEL)) &&
                b.cnt * 2 == a.cnt) {
                a.flags |= MF_FF | (cdl ? MF_FF_DL : 0);
                a.r_row = b.dst_row;
                a.tab2 = b.tab;
                a.pad1 = b.sh_dst;
                out.push_back(a);
                ++i;
                continue;
            }
        }
        out.push_back(a);
    }
    ops.swap(out);
}

// Fold the combine at depth n-5 into the right BOT3 before it (MF_BC2, the
// end of bot3_op in qpd_fast_bot.hpp): a right BOT3 that already runs its
// parent's combine (MF_BCOMB) and writes R[n-4] is followed by the COMB that
// reads that row and its left sibling's U[n-4]; the BOT3 computes that
// combine from its result in registers and writes the COMB's destination, so
// R[n-4] is neither stored nor loaded and the COMB op goes.  SCL-LUT only.
// pad1 of an MF_BC2 op: the folded combine's U pointer field, its destination's, and its destination
// row in the 16 bits above them -- read back with `pad1 >> 16` on the int32_t, so rows below 32768 only
inline int32_t bc2_pack(int sh_u, int sh_dst, int dst_row) {
    return (int32_t)((uint32_t)sh_u | ((uint32_t)sh_dst << 8) | ((uint32_t)dst_row << 16));
}

inline void fold_combine(std::vector<qpd::MOp> &ops) {
    using namespace qpd;
    std::vector<MOp> out;
    out.reserve(ops.size());
    for (size_t i = 0; i < ops.size(); ++i) {
        MOp a = ops[i];
        if (i + 1 < ops.size() && a.type == OP_BOT3 && (a.flags & MF_BCOMB) && (a.flags & MF_TO_R) && !(a.flags & MF_BC2)) {
            const MOp &b = ops[i + 1];
            if (b.type == OP_COMB && b.d == a.d - 2 && b.cnt == 16 && b.r_row == a.dst_row &&
                ((b.flags & MF_R_LDS) != 0) == ((a.flags & MF_DST_LDS) != 0) && b.sh_u < 256 && b.sh_dst < 256 &&
                b.dst_row >= 0 && b.dst_row < 32768) {
                a.flags |= MF_BC2 | ((b.flags & MF_U_LDS) ? MF_BC2_ULDS : 0) | ((b.flags & MF_DST_LDS) ? MF_BC2_DLDS : 0) |
                           ((b.flags & MF_TO_R) ? MF_BC2_TOR : 0);
                a.r_row = b.u_row;
                a.pad1 = bc2_pack(b.sh_u, b.sh_dst, b.dst_row);
                out.push_back(a);
                ++i;
                continue;
            }
        }
        out.push_back(a);
    }
    ops.swap(out);
}

// Place the global-slab drains (MF_SYNC: vmcnt(0) + barrier BEFORE the op).
// A path reads another path's slab rows only through pointer fields copied
// at a fork, and every op that writes a depth's rows writes all lanes' own
// columns and re-points them at themselves.  So a drain is needed only before
// an op that reads global rows through a pointer when some global write
// precedes a fork since the last drain; by then the stores have long
// completed and the drain costs almost nothing.  Single-path kinds (SC, Fast
// SC) never read another lane's rows.  A BOT3 with the parent's combine
// folded in (MF_BCOMB) reads U[n-3] through a pointer AFTER its own forks, so
// any global write before it is drained at its start.
inline void place_syncs(std::vector<qpd::MOp> &ops, bool list) {
    using namespace qpd;
    bool dirty = false, exposed = false;
    for (MOp &m : ops) {
        m.flags &= ~MF_SYNC;
        if (!list) continue;
        bool forks = false;
        switch (m.type) {
            case OP_BOT3: forks = m.cnt != 0xff; break;
            case OP_LEAF_L:
            case OP_LEAF_R: forks = m.cnt == 0; break;
            case OP_REP:
            case OP_R1: forks = true; break;
            default: break;
        }
        const bool src_glb = !(m.flags & (MF_SRC_LDS | MF_CHAN | MF_PRE));
        const bool spec_u = m.type >= OP_R0 && m.type <= OP_SPC && (m.flags & (MF_SGG | MF_SCOMB));
        const bool u_glb = ((m.type == OP_G || m.type == OP_COMB || m.type == OP_LEAF_R || spec_u ||
                             (m.type == OP_BOT3 && (m.flags & (MF_BG | MF_BCOMB)))) &&
                            !(m.flags & MF_U_LDS)) ||
                           (m.type == OP_BOT3 && (m.flags & MF_BC2) && !(m.flags & MF_BC2_ULDS));
        const bool late_u = (m.type == OP_BOT3 && forks &&
                             (((m.flags & MF_BCOMB) && !(m.flags & MF_U_LDS)) || ((m.flags & MF_BC2) && !(m.flags & MF_BC2_ULDS)))) ||
                            (forks && (m.flags & MF_SCOMB) && spec_u && !(m.flags & MF_U_LDS));
        if ((exposed && (src_glb || u_glb)) || (late_u && dirty)) {
            m.flags |= MF_SYNC;
            exposed = dirty = false;
        }
        if (!(m.flags & ((m.type == OP_BOT3 && (m.flags & MF_BC2)) ? MF_BC2_DLDS : MF_DST_LDS))) dirty = true;
        if (forks && dirty) exposed = true;
    }
}

// Row ownership of a fast layout: (space, row) -> slot (0 R, 1 S, 2 U) and tree
// depth, for the frozen-prefix split.
struct FastOwner {
    std::vector<int8_t> slot[2], depth[2];  // per space (0 slab, 1 LDS); slot -1: unowned
    void add(bool lds, int base, int cnt, int sl, int dd) {
        const int sp = lds ? 1 : 0;
        if ((int)slot[sp].size() < base + cnt) {
            slot[sp].resize(base + cnt, -1);
            depth[sp].resize(base + cnt, -1);
        }
        for (int r = 0; r < cnt; ++r) {
            slot[sp][base + r] = (int8_t)sl;
            depth[sp][base + r] = (int8_t)dd;
        }
    }
    int of(int sp, int row) const { return row >= 0 && row < (int)slot[sp].size() ? slot[sp][row] : -1; }
    int rows(int sp) const { return (int)slot[sp].size(); }
};

// Rows of the fast engine's slab / LDS an op reads and writes (space, first
// row, count), from the access pattern of its code in qpd_fast.hip and its headers.  Reads of
// the channel or a pre-pass row (MF_CHAN / MF_PRE) are not row reads.
template <class Fn>
void op_rows(const qpd::MOp &m, Fn &&acc) {
    using namespace qpd;
    const int fl = m.flags;
    const bool src_row = !(fl & (MF_CHAN | MF_PRE));
    const int sp_s = (fl & MF_SRC_LDS) ? 1 : 0, sp_u = (fl & MF_U_LDS) ? 1 : 0, sp_d = (fl & MF_DST_LDS) ? 1 : 0;
    const int c = m.cnt;
    switch (m.type) {
        case OP_F:
        case OP_G:
            if (src_row) acc(false, sp_s, m.src_row, c >= 8 ? 2 * (c >> 3) : 1);
            if (m.type == OP_G) acc(false, sp_u, m.u_row, std::max(1, c >> 5));
            acc(true, sp_d, m.dst_row, c >= 8 ? c >> 3 : 1);
            if (fl & MF_FF) acc(true, (fl & MF_FF_DL) ? 1 : 0, m.r_row, c >> 4);
            break;
        case OP_COMB: {
            const int cw = c < 32 ? 1 : c >> 5;
            acc(false, sp_u, m.u_row, cw);
            acc(false, (fl & MF_R_LDS) ? 1 : 0, m.r_row, cw);
            acc(true, sp_d, m.dst_row, c < 32 ? 1 : 2 * cw);
            break;
        }
        case OP_LEAF_L:
        case OP_LEAF_R:
            if (src_row) acc(false, sp_s, m.src_row, 1);
            if (m.type == OP_LEAF_R) acc(false, sp_u, m.u_row, 1);
            acc(true, sp_d, m.dst_row, 1);
            break;
        case OP_BOT3:
            if (src_row) acc(false, sp_s, m.src_row, (fl & MF_BFG) ? 2 : 1);
            if (fl & (MF_BG | MF_BCOMB)) acc(false, sp_u, m.u_row, 1);
            if (fl & MF_BC2) {
                acc(false, (fl & MF_BC2_ULDS) ? 1 : 0, m.r_row, 1);
                acc(true, (fl & MF_BC2_DLDS) ? 1 : 0, m.pad1 >> 16, 1);
            } else {
                acc(true, sp_d, m.dst_row, 1);
            }
            break;
        case OP_IMPORT: acc(true, sp_d, m.dst_row, c); break;
        case OP_EXPORT: acc(false, sp_s, m.src_row, c); break;
        default:  // special nodes: temp symbols in, temp bits out
            acc(false, sp_s, m.src_row, (c + 7) >> 3);
            acc(true, sp_d, m.dst_row, (c + 31) >> 5);
            break;
    }
}

// Frozen-prefix stages of an SCL schedule (see lut_prefix_kernel).
//   stage 1:  ops [0, s1) -- up to the first forking op: one path, gs = 1;
//   stage 1b: ops [s1, sb) -- up to the op with the second information leaf: at
//             most 2 live paths, run with L = 2, gs = 2 (opt-in: QPD_PFX1B=1);
//   stage 2:  ops [sb, s2) -- up to the op with the third information leaf: at
//             most 4 live paths, run with L = 4;
//   decode:   ops [s2, end) with the full list.
// For 2L <= 16 mink's sort is stable (SCLLUTDecoder.cpp:8-21, H1): the live
// candidates (keeps before flips, each in slot order) take slots 0..2k-1 in the
// same order at L = 2, 4 or 8, and the other slots' metrics are infinite.
// Each stage ends with OP_EXPORT of the words the later ops read before
// writing them (live-in) and begins with OP_IMPORT of its predecessor's.
// The stages' lists, record sizes and metric words go to FastHostPlan::pfx /
// pfx_rec / pfx_pm (stage 1, 1b, 2), the decode kernel's list to `rest`.

inline bool is_fork(const qpd::MOp &m) {
    using namespace qpd;
    return (m.type == OP_BOT3 && m.cnt != 0xff) || ((m.type == OP_LEAF_L || m.type == OP_LEAF_R) && m.cnt == 0) ||
           m.type == OP_R1 || m.type == OP_REP || m.type == OP_SPC;
}

inline int info_leaves(const qpd::MOp &m) {
    using namespace qpd;
    if (m.type == OP_BOT3) return __builtin_popcount(~m.cnt & 0xff);
    if (m.type == OP_LEAF_L || m.type == OP_LEAF_R) return m.cnt == 0;
    return 0;
}

// Live-in words of ops[from, end): live[sp][row].  False if an unowned row is read.
inline bool live_in(const std::vector<qpd::MOp> &ops, size_t from, const FastOwner &own, std::vector<char> (&live)[2]) {
    std::vector<char> def[2];
    for (int sp = 0; sp < 2; ++sp) {
        def[sp].assign(own.rows(sp), 0);
        live[sp].assign(own.rows(sp), 0);
    }
    bool ok = true;
    for (size_t i = from; i < ops.size() && ok; ++i)
        op_rows(ops[i], [&](bool wr, int sp, int row, int cnt) {
            for (int r = row; r < row + cnt; ++r) {
                if (own.of(sp, r) < 0) {
                    if (!wr) ok = false;
                    continue;
                }
                if (wr) def[sp][r] = 1;
                else if (!def[sp][r]) live[sp][r] = 1;
            }
        });
    return ok;
}

// Runs of live words with one slot and depth: fn(sp, first row, count, slot, depth).
template <class Fn>
void live_runs(const std::vector<char> (&live)[2], const FastOwner &own, Fn &&fn) {
    for (int sp = 0; sp < 2; ++sp)
        for (int r = 0; r < own.rows(sp);) {
            if (!live[sp][r]) {
                ++r;
                continue;
            }
            int e = r;
            while (e < own.rows(sp) && live[sp][e] && own.slot[sp][e] == own.slot[sp][r] && own.depth[sp][e] == own.depth[sp][r])
                ++e;
            fn(sp, r, e - r, (int)own.slot[sp][r], (int)own.depth[sp][r]);
            r = e;
        }
}

inline qpd::MOp blank_op(int type) {
    qpd::MOp m;
    std::memset(&m, 0, sizeof(m));
    m.type = type;
    return m;
}

inline bool plan_prefix(const std::vector<qpd::MOp> &ops, const FastOwner &own, int L, const PlanSwitches &sw, FastHostPlan &P,
                        std::vector<qpd::MOp> &rest) {
    using namespace qpd;
    size_t s1 = 0;
    while (s1 < ops.size() && !is_fork(ops[s1])) ++s1;
    if (s1 == 0 || s1 == ops.size()) return false;
    // stage 1 -> one-path records (geometry G = 6, PS = 0): S words (computed) and the
    // metric; U / R words are zeros (every decision of the prefix is a frozen 0)
    std::vector<char> live1[2];
    if (!live_in(ops, s1, own, live1)) return false;
    std::vector<MOp> imp1, exp1;
    int w1 = 0;
    live_runs(live1, own, [&](int sp, int r, int cnt, int slot, int) {
        MOp m = blank_op(OP_IMPORT);
        m.dst_row = r;
        m.cnt = cnt;
        m.flags = sp ? MF_DST_LDS : 0;
        if (slot == 1) {
            m.flags |= MF_XBUF;
            m.src_row = w1;
            MOp x = blank_op(OP_EXPORT);
            x.flags = sp ? MF_SRC_LDS : 0;
            x.src_row = r;
            x.dst_row = w1;
            x.cnt = cnt;
            exp1.push_back(x);
            w1 += cnt;
        } else {
            m.flags |= MF_ZERO;
        }
        imp1.push_back(m);
    });
    P.pfx_pm[0] = w1;
    P.pfx_rec[0] = w1 + 2;
    MOp pm = blank_op(OP_IMPORT);
    pm.flags = MF_XBUF | MF_PM;
    pm.src_row = P.pfx_pm[0];
    imp1.insert(imp1.begin(), pm);
    for (MOp &m : imp1) {  // record words, geometry and live paths; the address is patched per buffer
        m.tab = P.pfx_rec[0];
        m.vrow = 6;
        m.tab2 = 1;
        m.node = 1;  // buffer: stage 1's
    }
    P.pfx[0].assign(ops.begin(), ops.begin() + s1);
    P.pfx[0].insert(P.pfx[0].end(), exp1.begin(), exp1.end());
    // stage 2 (4 < L <= 8): up to the op with the third information leaf.  Not above L = 8:
    // mink's 2L > 16 candidates go through libstdc++'s introsort there, whose order of tied
    // live metrics the stable L = 4 selection would not reproduce (H1).
    size_t s2 = s1;
    for (int inf = 0; s2 < ops.size() && inf + info_leaves(ops[s2]) <= 2; ++s2) inf += info_leaves(ops[s2]);
    std::vector<char> live2[2];
    if (L <= 4 || L > qpd::kMaxL || sw.no_pfx2 || s2 <= s1 || s2 >= ops.size() || !live_in(ops, s2, own, live2)) {
        rest = imp1;
        rest.insert(rest.end(), ops.begin() + s1, ops.end());
        return true;
    }
    // stage 2 -> four-path records (G = 4, PS = 2), stage 1b -> two-path records (G = 5,
    // PS = 1): every live word, read through the lineage's pointer of its depth, and the metric
    auto path_records = [&](const std::vector<char> (&live)[2], int G, int PS, int node, std::vector<MOp> &imp,
                            std::vector<MOp> &exp, int &rec, int &pmw) {
        int w = 0;
        live_runs(live, own, [&](int sp, int r, int cnt, int slot, int dd) {
            MOp x = blank_op(OP_EXPORT);
            x.flags = (sp ? MF_SRC_LDS : 0) | (slot == 1 ? MF_VIA_PS : slot == 2 ? MF_VIA_PU : 0);
            x.sh_src = slot == 2 ? u_field(dd) : 4 * dd;
            x.src_row = r;
            x.dst_row = w;
            x.cnt = cnt;
            exp.push_back(x);
            MOp m = blank_op(OP_IMPORT);
            m.flags = MF_XBUF | (sp ? MF_DST_LDS : 0);
            m.src_row = w;
            m.dst_row = r;
            m.cnt = cnt;
            imp.push_back(m);
            w += cnt;
        });
        pmw = w;
        rec = w + 2;
        MOp pm = blank_op(OP_IMPORT);
        pm.flags = MF_XBUF | MF_PM;
        pm.src_row = pmw;
        imp.insert(imp.begin(), pm);
        for (MOp &m : imp) {
            m.tab = rec;
            m.vrow = G | (PS << 8);
            m.tab2 = 1 << PS;  // live paths of the record
            m.node = node;     // buffer: 2 stage 2's, 3 stage 1b's
        }
    };
    std::vector<MOp> imp2, exp2;
    path_records(live2, 4, 2, 2, imp2, exp2, P.pfx_rec[2], P.pfx_pm[2]);
    // stage 1b (opt-in, QPD_PFX1B=1): the ops up to the one with the second information
    // leaf, run by 2 lanes per frame instead of stage 2's 4 (a third of the stages' lane
    // lookups on the bench code).  Measured -0.7 % on the bench workload: stage 2 2.19 ->
    // 1.30 ms, but stage 1b's own launch, drain and records take 1.07 ms (profiles/r06m_*).
    size_t sb = s1;
    for (int inf = 0; sb < ops.size() && inf + info_leaves(ops[sb]) <= 1; ++sb) inf += info_leaves(ops[sb]);
    std::vector<char> liveb[2];
    if (sb > s1 && sb < s2 && sw.pfx1b && live_in(ops, sb, own, liveb)) {
        std::vector<MOp> impb, expb;
        path_records(liveb, 5, 1, 3, impb, expb, P.pfx_rec[1], P.pfx_pm[1]);
        P.pfx[1] = imp1;
        P.pfx[1].insert(P.pfx[1].end(), ops.begin() + s1, ops.begin() + sb);
        P.pfx[1].insert(P.pfx[1].end(), expb.begin(), expb.end());
        imp1 = impb;  // stage 2 starts from stage 1b's records
        s1 = sb;
    }
    P.pfx[2] = imp1;
    P.pfx[2].insert(P.pfx[2].end(), ops.begin() + s1, ops.begin() + s2);
    P.pfx[2].insert(P.pfx[2].end(), exp2.begin(), exp2.end());
    rest = imp2;
    rest.insert(rest.end(), ops.begin() + s2, ops.end());
    return true;
}

#ifndef QPD_DEFAULT_SETS
#define QPD_DEFAULT_SETS 2
#endif
constexpr int kDefaultSets = QPD_DEFAULT_SETS;

// The S-row and U-row pointer fields an op reads or sets, by op type (the
// access pattern of each op's code): fn(slot 0 = S / 1 = U, int &sh).  An
// MF_BC2 op's two fields, packed in pad1, are presented unpacked in bc_u / bc_dst.
template <class Fn>
void pointer_fields(qpd::MOp &m, int &bc_u, int &bc_dst, Fn &&fn) {
    using namespace qpd;
    bc_u = m.pad1 & 255;
    bc_dst = (m.pad1 >> 8) & 255;
    const int fl = m.flags;
    const bool src_row = !(fl & (MF_CHAN | MF_PRE));
    switch (m.type) {
        case OP_F:
        case OP_G:
            if (src_row) fn(0, m.sh_src);
            if (m.type == OP_G) fn(1, m.sh_u);  // (MF_GSEL reads U[1] through it too)
            fn(0, m.sh_dst);
            if (fl & MF_FF) fn(0, m.pad1);
            break;
        case OP_LEAF_L:
        case OP_LEAF_R:
            if (src_row) fn(0, m.sh_src);
            if (m.type == OP_LEAF_R) fn(1, m.sh_u);
            else fn(1, m.sh_dst);
            break;
        case OP_COMB:
            fn(1, m.sh_u);
            if (!(fl & MF_TO_R)) fn(1, m.sh_dst);
            break;
        case OP_BOT3:
            if (src_row) fn(0, m.sh_src);
            if (fl & (MF_BG | MF_BCOMB)) fn(1, m.sh_u);
            if (!(fl & MF_TO_R)) fn(1, m.sh_dst);
            if (fl & MF_BC2) {  // (the fields packed in pad1, unpacked into bc_u / bc_dst)
                fn(1, bc_u);
                if (!(fl & MF_BC2_TOR)) fn(1, bc_dst);
            }
            break;
        case OP_IMPORT: break;
        case OP_EXPORT:
            if (fl & MF_VIA_PS) fn(0, m.sh_src);
            if (fl & MF_VIA_PU) fn(1, m.sh_src);
            break;
        default:  // special nodes
            fn(0, m.sh_src);
            if (fl & (MF_SGG | MF_SCOMB)) fn(1, m.sh_u);
            if (!(fl & MF_TO_R)) fn(1, m.sh_dst);
            break;
    }
}

// One pointer word per path (PathT<true>, qpd_fast_select.hpp): the pointer fields
// the op lists use (pointer_fields), packed into consecutive 4-bit positions
// of one word.  False (lists unchanged) when they need more than 16 fields.
inline bool compact_pointer_fields(const std::vector<std::vector<qpd::MOp> *> &lists) {
    using namespace qpd;
    int pos[2][kMaxDepth + 1];
    for (auto &a : pos)
        for (int &x : a) x = -1;
    int bc_u = 0, bc_dst = 0;
    int used = 0;
    for (auto *l : lists)
        for (qpd::MOp &m : *l)
            pointer_fields(m, bc_u, bc_dst, [&](int sl, int &sh) {
                int &p = pos[sl][sh / 4];
                if (p < 0) p = used++;
            });
    if (used > 16) return false;
    for (auto *l : lists)
        for (qpd::MOp &m : *l) {
            // every field of an op is rewritten once (fields shared by two
            // roles, e.g. sh_src of a special node, are read before any write)
            int sh_src = m.sh_src, sh_u = m.sh_u, sh_dst = m.sh_dst, pad1 = m.pad1;
            int nbc_u = m.pad1 & 255, nbc_dst = (m.pad1 >> 8) & 255;
            pointer_fields(m, bc_u, bc_dst, [&](int sl, int &sh) {
                const int np = 4 * pos[sl][sh / 4];
                if (&sh == &m.sh_src) sh_src = np;
                else if (&sh == &m.sh_u) sh_u = np;
                else if (&sh == &m.pad1) pad1 = np;
                else if (&sh == &bc_u) nbc_u = np;
                else if (&sh == &bc_dst) nbc_dst = np;
                else sh_dst = np;
            });
            if (m.type == OP_BOT3 && (m.flags & MF_BC2)) pad1 = (m.pad1 & ~0xFFFF) | nbc_u | (nbc_dst << 8);
            m.sh_src = sh_src;
            m.sh_u = sh_u;
            m.sh_dst = sh_dst;
            m.pad1 = pad1;
        }
    return true;
}

// Rows of slot sl (0 = R, 1 = S, 2 = U) at depth dd of a code of N = 2^n symbols.
inline int slot_rows(int N, int n, int sl, int dd) {
    const int srows = std::max(1, (N >> dd) / 8), brows = std::max(1, (N >> dd) / 32);
    if (sl == 1) return (dd >= 1 && dd <= n - 1) ? srows : 0;
    if (sl == 2) return dd >= 1 ? brows : 0;
    return brows;
}

// Row ownership of layout Ly with the slots `use` keeps.
inline FastOwner make_owner(const FastLayout &Ly, const bool (&use)[3][qpd::kMaxDepth + 1], int N, int n) {
    FastOwner own;
    for (int dd = 0; dd <= n; ++dd)
        for (int sl = 0; sl < 3; ++sl) {
            const int b = sl == 0 ? Ly.R[dd] : sl == 1 ? Ly.S[dd] : Ly.U[dd];
            own.add(Ly.lds(dd), b, use[sl][dd] ? slot_rows(N, n, sl, dd) : 0, sl, dd);
        }
    return own;
}

// Nibble-packed tables: entry (u, a, b) of node p at bit 4*(idx&7) of dword idx>>3, idx =
// u * 256 + a * 16 + b; the leaf pairs' nodes (depth n-1: only the leaf lookups read them)
// transposed, idx = u * 256 + b * 16 + a (qpd_fast_bot.hpp leaf_idx, QPD_LEAF_T)
inline void pack_tables(const qpd_config &c, std::vector<uint32_t> &ft, std::vector<uint32_t> &gt) {
    const int N = c.N, v = c.v;
    ft.assign((size_t)(N - 1) * 32, 0);
    gt.assign((size_t)(N - 1) * 64, 0);
    const size_t vv = (size_t)v * v;
    for (int p = 0; p < N - 1; ++p) {
        const uint8_t *tf = c.lut_f + (size_t)c.f_base[p] * vv;
        const uint8_t *tg = c.lut_g + (size_t)c.g_base[p] * 2 * vv;
        const bool leafpair = QPD_LEAF_T && p >= (N >> 1) - 1;
        for (int a = 0; a < v; ++a)
            for (int b = 0; b < v; ++b) {
                const int idx = leafpair ? b * 16 + a : a * 16 + b;
                ft[(size_t)p * 32 + (idx >> 3)] |= (uint32_t)tf[a * v + b] << (4 * (idx & 7));
                for (int u = 0; u < 2; ++u) {
                    const int gi = u * 256 + idx;
                    gt[(size_t)p * 64 + (gi >> 3)] |= (uint32_t)tg[u * vv + a * v + b] << (4 * (gi & 7));
                }
            }
    }
}

// The fast plan of code c (kind: the kernel family; N = 2^n; list size L, 1 for
// the SC kinds) with schedule s.  QPD_OK, or a refusal with its message in err.
inline int plan_fast(const qpd_config &c, int n, int L, const Schedule &s, const PlanSwitches &sw, FastHostPlan &P,
                     std::string &err) {
    const int N = c.N, v = c.v;
    // Row slots per depth: 0 = R, 1 = S, 2 = U.  `use` keeps all of them, or
    // (trimmed layout) only those some op touches: BOT3 subtrees keep depths
    // n-2..n in registers and the fused BOT3s also skip S/R[n-3], which frees
    // LDS for a shallower lds_from.
    bool(&use)[3][qpd::kMaxDepth + 1] = P.use;
    for (auto &u : use)
        for (bool &b : u) b = true;
    auto assign = [&](FastLayout &Lt, int &rl, int &rg) {
        rl = rg = 0;
        for (int dd = 0; dd <= n; ++dd) {  // grouped by depth (see FastLayout)
            int &r = Lt.lds(dd) ? rl : rg;
            if (Lt.lds(dd)) Lt.lds_base[dd] = r;
            for (int sl = 0; sl < 3; ++sl) {
                (sl == 0 ? Lt.R : sl == 1 ? Lt.S : Lt.U)[dd] = r;
                if (use[sl][dd]) r += slot_rows(N, n, sl, dd);
            }
        }
        Lt.lds_base[n + 1] = rl;
        Lt.lds_end = rl + qpd::kSelInts / 64;
    };
    const bool list_kind = c.kind == QPD_SCL_LUT || c.kind == QPD_FASTSCL_LUT;
    // one frame set for FastSC-LUT (N=1024: 171 -> 241 M frames/s with one set,
    // profiles/r03z_sets.txt); two for the list kinds, FastSCL-LUT included (round 5:
    // the SCL-LUT kernel's two-set machinery with the special-node ops)
    P.sets = c.kind == QPD_FASTSC_LUT ? 1 : kDefaultSets;
    if (sw.sets) P.sets = sw.sets < 3 ? sw.sets : (c.kind == QPD_SCL_LUT && L == 8) ? 3 : 2;
    P.l8 = list_kind && L == 8;
    // lane groups of 16: SCL-LUT, and FastSCL-LUT where the fast engine was asked for (qpd_create:
    // AUTO keeps it on the generic engine).  FastSCL-LUT's W16 plan has no mixed bottom subtrees
    // and no folded special nodes (Ly.botx below: both are L = 8 code), its special nodes run
    // through the single-set special_op, one frame set after the other.
    P.w16 = list_kind && L > qpd::kMaxL;
    const int NS = P.sets;
    FastLayout &Ly = P.layout;
    Ly = FastLayout();
    Ly.ns = NS;
    const int32_t *nt_fast = (c.kind == QPD_FASTSC_LUT || c.kind == QPD_FASTSCL_LUT) ? c.node_type : nullptr;
    auto ops_on = [&](const FastLayout &Lt, std::vector<qpd::MOp> &out, std::vector<uint16_t> &r1) {
        fast_ops(out, Lt, sw, c.kind, N, n, v, c.frozen_bits, nt_fast, c.vcl, r1, 0, 0);
    };
    // pre-mode: S[1] is whole words (N >= 16) and the root's left child a plain node
    Ly.pre = n >= 4 && special_of(c.kind, nt_fast, 1) < 0 && !sw.no_pre;
    Ly.bfuse = !sw.no_bfuse;
    Ly.botx = c.kind == QPD_FASTSCL_LUT && P.l8 && !sw.no_botx;
    // Trimmed layout: probe the op list on an all-global layout and keep the
    // slots whose rows it touches (op_rows).  (FastSCL's R1 argsorts of > 16
    // elements borrow the LDS tail of the deeper levels; it is padded below
    // where it is too short.)
    if (!sw.no_trim) {
        FastLayout Lp = Ly;
        Lp.D = n + 1;
        int pl = 0, pg = 0;
        assign(Lp, pl, pg);
        std::vector<qpd::MOp> probe;
        std::vector<uint16_t> r1p;
        ops_on(Lp, probe, r1p);
        const FastOwner own = make_owner(Lp, use, N, n);
        bool used[3][qpd::kMaxDepth + 1] = {};
        for (const qpd::MOp &m : probe)
            op_rows(m, [&](bool, int sp, int row, int cnt) {
                for (int r = row; r < row + cnt; ++r)
                    if (own.of(sp, r) >= 0) used[own.slot[sp][r]][own.depth[sp][r]] = true;
            });
        used[0][0] = true;  // R[0]: the tail re-encodes it
        std::memcpy(use, used, sizeof(use));
    }
    // the list kinds' byte tables of the f / g ops at two frame sets (stage_tab in
    // qpd_fast_lookup.hpp: 512 B for the op's table, 256 B for a folded child's f), at LDS
    // offset 0: before the sets' rows and selection scratch (lut_lds)
    P.lds_tab_bytes = list_kind && NS >= 2 ? 768 : 0;
    // LDS per wave = NS * (selection scratch + rows of depths >= D) + the byte
    // tables; the budget is measured: occupancy beats LDS residency of the
    // shallow depths.
    P.lds_budget = sw.lds_budget != PlanSwitches::kUnset ? sw.lds_budget : NS == 1 ? 6 * 1024 : NS == 2 ? 10 * 1024 : 15 * 1024;
    // FastSCL R1 nodes of 17..32 elements sort in the wave's LDS tail of the
    // deeper levels (MF_R1_LDS): rows of padding so that the tail holds cnt / 2
    // rows -- part of the LDS the budget bounds
    auto r1_pad = [&](const FastLayout &Lt) {
        int pad = 0;
        for (const qpd::Op &o : s.ops)
            if (c.kind == QPD_FASTSCL_LUT && o.type == qpd::OP_R1 && (N >> o.d) > qpd::stl::kThreshold &&
                (N >> o.d) <= 32 && Lt.lds(o.d + 1)) {
                const int have = NS * (Lt.lds_end - Lt.lds_base[o.d + 1]), need = (N >> o.d) / 2;
                if (have < need) pad = std::max(pad, (need - have + NS - 1) / NS);
            }
        return pad;
    };
    int rl = 0, rg = 0;
    for (;; ++Ly.D) {
        assign(Ly, rl, rg);
        const int pad = r1_pad(Ly);
        if (Ly.D > n || NS * (qpd::kSelInts * 4 + (rl + pad) * 256) + P.lds_tab_bytes <= P.lds_budget) {
            rl += pad;
            Ly.lds_end += pad;
            break;
        }
    }
    P.lds_from = Ly.D;
    P.R0_row = Ly.R[0];
    P.R0_lds = Ly.lds(0);
    P.H_row = P.K_row = P.I_row = rg;
    if (c.kind == QPD_FASTSCL_LUT && s.max_r1 > 0) {
        P.H_row = rg;
        rg += (s.max_r1 + 31) / 32;
        P.K_row = rg;
        rg += 2 * s.max_r1;
        P.I_row = rg;
        if (s.max_r1 > qpd::stl::kThreshold) rg += s.max_r1;
    }
    P.lds_rows = rl;
    P.glb_rows = std::max(rg, 1);
    P.lds_bytes = NS * (qpd::kSelInts * 4 + rl * 256) + P.lds_tab_bytes;
    P.pre = Ly.pre;
    // <= 8 GB of pre-pass rows (N bytes per frame) per chunk, 2^23 frames at N = 1024:
    // one decode launch, one drain and one set of prefix-stage launches per chunk (each
    // decode launch ends in a drain where its SIMDs idle one by one, so fewer, larger
    // launches are faster -- SCL-LUT bench workload: 2 GB chunks 53.5 M frames/s at 2^22
    // frames per call, 4 GB 54.3 M; at 2^23 4 GB 54.8 M, 8 GB 55.2 M --
    // profiles/r06q_ab_chunk.txt)
    P.pre_chunk = sw.pre_chunk ? sw.pre_chunk : std::max<int64_t>(1, ((int64_t)8 << 30) / N);
    std::vector<qpd::MOp> &mops = P.ops;
    mops.clear();
    P.r1tab.clear();
    ops_on(Ly, mops, P.r1tab);
    if (P.r1tab.empty()) P.r1tab.push_back(0);
    // Frozen-prefix stages (lut_prefix_kernel, plan_prefix): SCL-LUT in pre-mode.
    // FastSCL's R0 / REP nodes already take most of the prefix (4 ops of the bench
    // code; the one-stage split measured -3 % there, profiles/r03ab_*).
    for (int k = 0; k < 3; ++k) {
        P.pfx[k].clear();
        P.pfx_rec[k] = P.pfx_pm[k] = 0;
    }
    // The split needs every live path metric finite: stage 2 and the decode
    // kernel seed the dead slots with path 0's rows and +inf, where the
    // reference holds copies of other dead paths (SCLLUTDecoder.cpp:117-144);
    // the two agree while no live metric reaches +inf and ties with a dead one.
    // A metric is a sum of at most N leaf quanta (row n-1), so quanta below
    // DBL_MAX / 2N keep it finite; tables beyond that decode unsplit, exactly
    // as the reference does with its infinities.
    double qmax = 0.0;
    for (size_t i = (size_t)(n - 1) * N * v; i < (size_t)n * N * v; ++i) qmax = std::max(qmax, std::fabs(c.vcl[i]));
    const bool pm_finite = qmax <= __DBL_MAX__ / (2.0 * N);
    if (Ly.pre && L > 1 && c.kind == QPD_SCL_LUT && pm_finite && !sw.no_pfx) {
        std::vector<qpd::MOp> rest;
        if (plan_prefix(mops, make_owner(Ly, use, N, n), L, sw, P, rest)) mops.swap(rest);
    }
    // prefix_kernel() instantiates NS = 1 and 2 only: fast_launch's task count
    // (fgroups) must use the NS the launched kernel has
    P.pfx_sets = std::min(P.sets, 2);
    if (sw.pfx_sets) P.pfx_sets = std::min(P.pfx_sets, sw.pfx_sets);
    const std::vector<std::vector<qpd::MOp> *> lists = {&mops, &P.pfx[0], &P.pfx[1], &P.pfx[2]};
    // Rows in lookup order (QPD_ROW_BYTEIDX, qpd_fast_switches.hpp): the plain kinds, whose S rows of
    // >= 8 symbols only f / g ops and BOT3s read.  Row sizes, slots and pointers are what they were;
    // only the order of a row's nibbles changes, which every op of the plan then agrees on.
    P.row_lo = QPD_ROW_BYTEIDX != 0 && (c.kind == QPD_SC_LUT || c.kind == QPD_SCL_LUT);
    if (P.row_lo)
        for (auto *l : lists)
            for (qpd::MOp &m : *l)
                if (m.type == qpd::OP_F || m.type == qpd::OP_G || m.type == qpd::OP_BOT3) m.flags |= qpd::MF_LO;
    for (auto *l : lists) {
        // folded descents: the list kernels with two frame sets (ff_op)
        if (list_kind && !sw.no_ff && (l == &mops ? P.sets : P.pfx_sets) == 2) fuse_descent(*l);
        if (list_kind && !sw.no_bc2) fold_combine(*l);  // folded depth n-5 combines (any NS)
        place_syncs(*l, l != &mops || list_kind);
    }
    // Special nodes the lean code of the R1L = false kernels cannot take: R1 nodes of > 16
    // elements without their LDS tail (r1_large), or (L = 8) R1 nodes without ranks in the
    // op record and R0 / REP nodes without one quanta row
    P.r1l = false;
    for (const qpd::MOp &m : mops)
        if (c.kind == QPD_FASTSCL_LUT &&
            ((m.type == qpd::OP_R1 &&
              ((m.cnt > qpd::stl::kThreshold && !(m.flags & qpd::MF_R1_LDS)) || (P.l8 && !(m.flags & qpd::MF_R1_RK)))) ||
             (P.l8 && (m.type == qpd::OP_R0 || m.type == qpd::OP_REP) && !(m.flags & qpd::MF_VUNI))))
            P.r1l = true;
    // the W16 FastSCL-LUT kernels have no r1_large: such a plan is not served (the generic engine decodes it)
    if (c.kind == QPD_FASTSCL_LUT && P.w16 && P.r1l) {
        err = "fast engine, FastSCL-LUT with L > 8: an R1 node of more than 32 elements, or of more than 16 "
              "without room for its argsort in LDS, is not served (use the generic engine)";
        return QPD_E_UNSUPPORTED;
    }
    // one pointer word: the list kinds at one or two frame sets (the instantiations
    // fast_kernel() has); FastSCL-LUT only at two sets with L = 8 and no r1_large, or W16
    // (SCL-LUT only with the root pre-pass: those kernels have no channel reads, lut_fast_kernel kChan)
    const bool pw1_ok = c.kind == QPD_SCL_LUT ? NS <= 2 && Ly.pre
                                              : (c.kind == QPD_FASTSCL_LUT && ((NS == 2 && P.l8 && !P.r1l) || P.w16));
    P.pw1 = pw1_ok && !sw.no_pw1 && compact_pointer_fields(lists);
    for (const qpd::MOp &m : mops)  // the kernel's f / g ops have no (S[d] in LDS, S[d+1] in the slab) variant
        if ((m.type == qpd::OP_F || m.type == qpd::OP_G) && (m.flags & qpd::MF_SRC_LDS) && !(m.flags & qpd::MF_DST_LDS)) {
            err = "fast plan: an f/g op reads LDS rows and writes slab rows";
            return QPD_E_INVALID;
        }
    pack_tables(c, P.ft, P.gt);
    return QPD_OK;
}

}  // namespace qpd_plan
