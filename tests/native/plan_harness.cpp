// Test harness (CPU): the fast engine's plan compiler (csrc/qpd_plan.hpp)
// built with g++ beside the tests.  ph_check plans one configuration the way
// qpd_create does (family, schedule, plan_fast) and verifies what the kernels
// of qpd_fast.hip rely on and nothing on the device checks: every row an op
// touches lies inside its space and in a slot the layout kept, the R1 argsort
// scratch fits, the LDS size is what the launch allocates, the packed pointer
// fields fit one word, the prefix stages' imports stay inside the exporting
// stage's records, and planning is deterministic.
#include <cstdio>

#include "qpd_plan.hpp"

namespace {

using namespace qpd_plan;
using qpd::MOp;

struct Fail {
    std::string msg;
    bool ok = true;
    void operator()(const char *list, size_t i, const MOp &m, const std::string &what) {
        if (!ok) return;
        ok = false;
        char b[256];
        snprintf(b, sizeof b, "%s op %zu (type %d, d %d, node %d, flags 0x%x): ", list, i, m.type, m.d, m.node, m.flags);
        msg = b + what;
    }
    void operator()(const std::string &what) {
        if (ok) msg = what;
        ok = false;
    }
};

template <class T>
bool same(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(T)));
}

bool same_plan(const FastHostPlan &a, const FastHostPlan &b) {
    bool eq = same(a.ops, b.ops) && same(a.r1tab, b.r1tab) && same(a.ft, b.ft) && same(a.gt, b.gt);
    for (int k = 0; k < 3; ++k) eq = eq && same(a.pfx[k], b.pfx[k]) && a.pfx_rec[k] == b.pfx_rec[k] && a.pfx_pm[k] == b.pfx_pm[k];
    const int sa[] = {a.lds_from, a.lds_rows, a.glb_rows, a.R0_row, a.R0_lds, a.H_row, a.K_row, a.I_row, a.lds_bytes,
                      a.lds_tab_bytes, a.lds_budget, a.sets, a.pfx_sets, a.l8, a.w16, a.r1l, a.pw1, a.pre};
    const int sb[] = {b.lds_from, b.lds_rows, b.glb_rows, b.R0_row, b.R0_lds, b.H_row, b.K_row, b.I_row, b.lds_bytes,
                      b.lds_tab_bytes, b.lds_budget, b.sets, b.pfx_sets, b.l8, b.w16, b.r1l, b.pw1, b.pre};
    const FastLayout &x = a.layout, &y = b.layout;
    return eq && !std::memcmp(sa, sb, sizeof sa) && a.pre_chunk == b.pre_chunk && !std::memcmp(a.use, b.use, sizeof a.use) &&
           x.D == y.D && !std::memcmp(x.S, y.S, sizeof x.S) && !std::memcmp(x.U, y.U, sizeof x.U) &&
           !std::memcmp(x.R, y.R, sizeof x.R) && !std::memcmp(x.lds_base, y.lds_base, sizeof x.lds_base) &&
           x.lds_end == y.lds_end && x.pre == y.pre && x.bfuse == y.bfuse && x.ns == y.ns && x.botx == y.botx;
}

// The kernels' unpack expressions of the values the plan packs into part of a
// record word, each as the kernel writes it (on the int32_t field of the record).
//   MF_BC2's pad1, the end of bot3_op (qpd_fast_bot.hpp): `const int e = op.pad1;` then
//   `pfield(st[s].U(), e & 255)`, `M[s].st(op.flags & MF_BC2_DLDS, e >> 16, lane, res)` and
//   `pset(st[s].U(), (e >> 8) & 255, gl)`
inline int bc2_u_field(int32_t e) { return e & 255; }
inline int bc2_dst_field(int32_t e) { return (e >> 8) & 255; }
inline int bc2_dst_row(int32_t e) { return e >> 16; }
//   MF_R1_RK's rank and sign words, rank_of in r1_prep (qpd_fast_special.hpp):
//   `RK = ((uint64_t)(uint32_t)op.tab2 << 32) | (uint32_t)op.r_row` and
//   `((uint32_t)(RK >> (4 * sym)) & 15u) << 1 | (((uint32_t)op.pad1 >> sym) & 1u)`
inline uint32_t r1rk_entry(const qpd::MOp &m, int sym) {
    const uint64_t RK = ((uint64_t)(uint32_t)m.tab2 << 32) | (uint32_t)m.r_row;
    return ((uint32_t)(RK >> (4 * sym)) & 15u) << 1 | (((uint32_t)m.pad1 >> sym) & 1u);
}
//   a pointer field, pfield / pset (qpd_fast_lookup.hpp): `(p >> sh) & 15u` and `15ull << sh` on the
//   path's 64-bit pointer word (PathT, qpd_fast_select.hpp: uint64_t ps, pu; one word of them on a PW1
//   plan), so a field is a whole nibble of that word
inline bool field_in_word(int sh) { return sh >= 0 && sh % 4 == 0 && sh + 4 <= 64; }

// Every packed value of op m comes back from the kernel's unpack expression as the value the plan
// meant: the pointer fields (pointer_fields presents an MF_BC2 op's two packed ones unpacked, by the
// expressions above), an MF_BC2 op's result row `bc2_row` (the caller's: what the layout says the
// folded combine writes), an MF_R1_RK op's ranks and signs (`r1`: the node's rank keys, or null).
// The empty string, or what does not round-trip.
std::string check_packed(const qpd::MOp &m, int bc2_row, const uint16_t *r1, int v) {
    using namespace qpd;
    std::string bad;
    MOp t = m;
    int bc_u = 0, bc_dst = 0;
    pointer_fields(t, bc_u, bc_dst, [&](int, int &sh) {
        if (bad.empty() && !field_in_word(sh)) bad = "pointer field at shift " + std::to_string(sh) + " is not a nibble of a 64-bit word";
    });
    if (!bad.empty()) return bad;
    if (m.type == OP_BOT3 && (m.flags & MF_BC2)) {
        if (bc_u != bc2_u_field(m.pad1) || bc_dst != bc2_dst_field(m.pad1)) return "pointer_fields and the kernel unpack pad1 differently";
        if (bc2_dst_row(m.pad1) != bc2_row)
            return "pad1 >> 16 gives row " + std::to_string(bc2_dst_row(m.pad1)) + ", the plan packed row " + std::to_string(bc2_row);
    }
    if ((m.flags & MF_R1_RK) && r1)
        for (int sy = 0; sy < v; ++sy)
            if (r1rk_entry(m, sy) != r1[sy])
                return "rank key of symbol " + std::to_string(sy) + " unpacks to " + std::to_string(r1rk_entry(m, sy)) + ", the rank table has " +
                       std::to_string(r1[sy]);
    return bad;
}

void check_plan(const qpd_config &c, int n, const Schedule &s, const FastHostPlan &P, Fail &fail) {
    using namespace qpd;
    const int N = c.N;
    const FastOwner own = make_owner(P.layout, P.use, N, n);
    const std::vector<MOp> *lists[4] = {&P.pfx[0], &P.pfx[1], &P.pfx[2], &P.ops};
    const char *names[4] = {"stage 1", "stage 1b", "stage 2", "main"};
    const int stage_of_node[4] = {-1, 0, 2, 1};  // an import's buffer (op.node: 1 / 2 / 3) -> the exporting stage
    for (int li = 0; li < 4; ++li)
        for (size_t i = 0; i < lists[li]->size(); ++i) {
            const MOp &m = (*lists[li])[i];
            // rows inside their space, in a slot the layout kept
            op_rows(m, [&](bool wr, int sp, int row, int cnt) {
                const int lim = sp ? P.lds_rows : P.glb_rows;
                if (row < 0 || cnt < 0 || row + cnt > lim)
                    fail(names[li], i, m, std::string(wr ? "writes" : "reads") + " rows [" + std::to_string(row) + ", " +
                                              std::to_string(row + cnt) + ") of " + (sp ? "LDS" : "the slab") + ", which has " +
                                              std::to_string(lim));
                for (int r = row; r < row + cnt; ++r)
                    if (own.of(sp, r) < 0)
                        fail(names[li], i, m, std::string(wr ? "writes" : "reads") + " row " + std::to_string(r) + " of " +
                                                  (sp ? "LDS" : "the slab") + ": no slot the layout kept");
            });
            // the R1 argsort's LDS tail
            if ((m.flags & MF_R1_LDS) && (m.u_row < 0 || P.sets * (P.layout.lds_end - m.u_row) < m.cnt / 2))
                fail(names[li], i, m, "R1 argsort tail from LDS row " + std::to_string(m.u_row) + " is shorter than cnt / 2 rows");
            // the unservable f / g shape
            if ((m.type == OP_F || m.type == OP_G) && (m.flags & MF_SRC_LDS) && !(m.flags & MF_DST_LDS))
                fail(names[li], i, m, "f/g op reads LDS rows and writes slab rows");
            // packed values: every pointer field a nibble of the path's word (one word or two), and what
            // the kernel unpacks is what the plan packed.  An MF_BC2 op writes the row of its grandparent
            // (depth d - 2): R if that is a right child, else U, in LDS where the layout has that depth
            {
                const int gd = m.d - 2;
                const bool bc2 = m.type == OP_BOT3 && (m.flags & MF_BC2);
                if (bc2 && (gd < 0 || ((m.flags & MF_BC2_DLDS) != 0) != P.layout.lds(gd)))
                    fail(names[li], i, m, "MF_BC2: the result row's space is not the layout's of depth d - 2");
                const int row = !bc2 || gd < 0 ? 0 : (m.flags & MF_BC2_TOR) ? P.layout.R[gd] : P.layout.U[gd];
                const bool own_tab = m.type == OP_R1 && !(m.flags & MF_SFG) && m.tab >= 0 && (size_t)m.tab + c.v <= P.r1tab.size();
                const std::string bad = check_packed(m, row, own_tab ? P.r1tab.data() + m.tab : nullptr, c.v);
                if (!bad.empty()) fail(names[li], i, m, bad);
            }
            // prefix records
            if (m.type == OP_IMPORT && (m.flags & MF_XBUF)) {
                const int st = m.node >= 1 && m.node <= 3 ? stage_of_node[m.node] : -1;
                const int words = (m.flags & MF_PM) ? 2 : m.cnt;
                if (st < 0 || st >= li || P.pfx[st].empty())
                    fail(names[li], i, m, "import from a stage that does not run before this list");
                else if (m.tab != P.pfx_rec[st] || m.src_row < 0 || m.src_row + words > P.pfx_rec[st])
                    fail(names[li], i, m, "import reads words past the exporting stage's record");
            }
            if (m.type == OP_EXPORT && (li == 3 || m.dst_row < 0 || m.dst_row + m.cnt > P.pfx_pm[li]))
                fail(names[li], i, m, "export outside the stage's record words");
        }
    for (int k = 0; k < 3; ++k)
        if (!P.pfx[k].empty() && (P.pfx_pm[k] < 0 || P.pfx_pm[k] + 2 > P.pfx_rec[k]))
            fail("stage " + std::to_string(k) + ": metric words outside the record");
    // R1 slab scratch after the rows, inside the slab
    if (own.rows(0) > P.H_row || P.H_row > P.K_row || P.K_row > P.I_row || P.I_row > P.glb_rows)
        fail("R1 slab scratch rows out of order");
    if (c.kind == QPD_FASTSCL_LUT && s.max_r1 > 0 &&
        (P.H_row + (s.max_r1 + 31) / 32 > P.K_row || P.K_row + 2 * s.max_r1 > P.I_row ||
         P.I_row + (s.max_r1 > qpd::stl::kThreshold ? s.max_r1 : 0) > P.glb_rows))
        fail("R1 slab scratch (H / K / I rows for max_r1 = " + std::to_string(s.max_r1) + ") outside the slab");
    // LDS size
    if (own.rows(1) > P.lds_rows || P.layout.lds_end != P.lds_rows + kSelInts / 64)
        fail("LDS rows: the layout's rows and selection scratch do not match lds_rows");
    if (P.lds_bytes != P.sets * (kSelInts * 4 + P.lds_rows * 256) + P.lds_tab_bytes) fail("lds_bytes is not sets * (scratch + rows) + tables");
    if (P.lds_from <= n && P.lds_bytes > P.lds_budget)
        fail("lds_bytes " + std::to_string(P.lds_bytes) + " over the budget " + std::to_string(P.lds_budget));
}

}  // namespace

extern "C" int ph_switches_size(void) { return (int)sizeof(qpd_plan::PlanSwitches); }

// Self-test of check_packed: plans cfg, takes a copy of its first MF_BC2 record, packs `dst_row`
// into the copy as fold_combine does (bc2_pack) and runs the check on it.  0: the copy round-trips;
// 1: the check fails (msg); -1: the plan has no MF_BC2 op; -2: no plan.
extern "C" int ph_pack_selftest(const qpd_config *cfg, const qpd_plan::PlanSwitches *sw, int dst_row, char *msg, int msg_len) {
    int fam = 0, dom = 0, n = 0;
    msg[0] = 0;
    if (!qpd_sched::family_of(cfg->kind, &fam, &dom) || dom != qpd::DOM_LUT) return -2;
    qpd_config c = *cfg;
    c.kind = fam;
    while ((1 << n) < c.N) ++n;
    Schedule s;
    qpd_sched::visit(s, fam, c.N, n, c.frozen_bits, nullptr, 0, 0);
    FastHostPlan P;
    std::string err;
    if (plan_fast(c, n, c.L, s, *sw, P, err)) return -2;
    for (const MOp &m : P.ops)
        if (m.type == qpd::OP_BOT3 && (m.flags & qpd::MF_BC2)) {
            MOp t = m;
            t.pad1 = bc2_pack(bc2_u_field(m.pad1), bc2_dst_field(m.pad1), dst_row);
            const std::string bad = check_packed(t, dst_row, nullptr, c.v);
            snprintf(msg, msg_len, "%s", bad.c_str());
            return bad.empty() ? 0 : 1;
        }
    return -1;
}

// 0: planned and every invariant holds; 1: an invariant fails; < 0: plan_fast's
// refusal (its code); -100: not a fast-engine configuration.  msg: the failure
// or refusal.  stats: lds_from, main ops, prefix ops, pw1, r1l, the or of all
// ops' flags, sets, w16.
extern "C" int ph_check(const qpd_config *cfg, const qpd_plan::PlanSwitches *sw, char *msg, int msg_len, int32_t *stats) {
    int fam = 0, dom = 0;
    msg[0] = 0;
    if (!qpd_sched::family_of(cfg->kind, &fam, &dom) || dom != qpd::DOM_LUT || cfg->f_step || cfg->g_step || cfg->v > 16) return -100;
    qpd_config c = *cfg;
    c.kind = fam;
    int n = 0;
    while ((1 << n) < c.N) ++n;
    const bool list = fam == QPD_SCL_LUT || fam == QPD_FASTSCL_LUT;
    const int L = list ? c.L : 1;
    if (L > 2 * qpd::kMaxL) return -100;
    Schedule s;
    qpd_sched::visit(s, fam, c.N, n, c.frozen_bits, (fam == QPD_FASTSC_LUT || fam == QPD_FASTSCL_LUT) ? c.node_type : nullptr, 0, 0);
    FastHostPlan P, Q;
    std::string err, err2;
    const int rc = plan_fast(c, n, L, s, *sw, P, err);
    Fail fail;
    if (plan_fast(c, n, L, s, *sw, Q, err2) != rc || err != err2 || (!rc && !same_plan(P, Q))) fail("planning twice gives different plans");
    if (!rc) check_plan(c, n, s, P, fail);
    snprintf(msg, msg_len, "%s", fail.ok ? err.c_str() : fail.msg.c_str());
    if (!fail.ok) return 1;
    if (rc) return rc;
    int flags = 0;
    for (const auto *l : {&P.ops, &P.pfx[0], &P.pfx[1], &P.pfx[2]})
        for (const MOp &m : *l) flags |= m.flags;
    const int32_t st[8] = {P.lds_from, (int32_t)P.ops.size(), (int32_t)(P.pfx[0].size() + P.pfx[1].size() + P.pfx[2].size()),
                           P.pw1, P.r1l, flags, P.sets, P.w16};
    std::memcpy(stats, st, sizeof st);
    return 0;
}
