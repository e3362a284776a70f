// Test harness (CPU): the fast engine's plan compiler (csrc/qpd_plan.hpp) built with g++
// beside the tests, for tests/test_plan_row_order.py.  pro_plan plans one configuration the
// way qpd_create does (family, schedule, plan_fast) and hands out the op lists as they
// are -- the prefix stages' and the decode kernel's, 16 int32 per record (qpd::MOp) -- for
// the test's symbolic walk of the rows' nibble order.  Built twice by the test: as the
// product (QPD_ROW_BYTEIDX from qpd_fast_switches.hpp) and with -DQPD_ROW_BYTEIDX=0.
#include <cstdio>

#include "qpd_plan.hpp"

using namespace qpd_plan;

static_assert(sizeof(qpd::MOp) == 16 * sizeof(int32_t), "an op record is 16 int32");

// The lists of the plan in the order they run: list 0 = stage 1, 1 = stage 1b, 2 = stage 2,
// 3 = the decode kernel.  `ops` receives the records of all lists back to back (room for
// `cap` records), `counts[4]` their lengths, `info[4]` = {row_lo, pre, sets, lds_from}.
// Returns the number of records, -1 when `cap` is too small, -2 when the plan is refused,
// -100 when the configuration is not the fast engine's.
extern "C" int pro_plan(const qpd_config *cfg, const PlanSwitches *sw, int32_t *ops, int cap, int32_t *counts, int32_t *info) {
    int fam = 0, dom = 0;
    if (!qpd_sched::family_of(cfg->kind, &fam, &dom) || dom != qpd::DOM_LUT || cfg->f_step || cfg->g_step || cfg->v > 16) return -100;
    qpd_config c = *cfg;
    c.kind = fam;
    int n = 0;
    while ((1 << n) < c.N) ++n;
    const bool list = fam == QPD_SCL_LUT || fam == QPD_FASTSCL_LUT;
    const int L = list ? c.L : 1;
    Schedule s;
    qpd_sched::visit(s, fam, c.N, n, c.frozen_bits, (fam == QPD_FASTSC_LUT || fam == QPD_FASTSCL_LUT) ? c.node_type : nullptr, 0, 0);
    FastHostPlan P;
    std::string err;
    if (plan_fast(c, n, L, s, *sw, P, err)) return -2;
    const std::vector<qpd::MOp> *lists[4] = {&P.pfx[0], &P.pfx[1], &P.pfx[2], &P.ops};
    int total = 0;
    for (int k = 0; k < 4; ++k) {
        counts[k] = (int32_t)lists[k]->size();
        total += counts[k];
    }
    if (total > cap) return -1;
    int at = 0;
    for (int k = 0; k < 4; ++k)
        for (const qpd::MOp &m : *lists[k]) std::memcpy(ops + 16 * at++, &m, sizeof m);
    info[0] = P.row_lo;
    info[1] = P.pre;
    info[2] = P.sets;
    info[3] = P.lds_from;
    return total;
}

extern "C" int pro_switches_size(void) { return (int)sizeof(PlanSwitches); }
extern "C" int pro_row_byteidx(void) { return QPD_ROW_BYTEIDX; }
