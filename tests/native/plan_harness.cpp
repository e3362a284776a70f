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
            // one pointer word: every field the op uses is a nibble position of it
            if (P.pw1) {
                MOp t = m;
                int bc_u = 0, bc_dst = 0;
                pointer_fields(t, bc_u, bc_dst, [&](int, int &sh) {
                    if (sh < 0 || sh >= 64 || sh % 4) fail(names[li], i, m, "pointer field " + std::to_string(sh) + " outside one word");
                });
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
