// Test harness (CPU): qpd_decode_list_host's host-engine branch without a device --
// the argument rules (qpd_list.hpp: check) and the host engine's list run (host_run)
// exactly as qpd_capi.hip calls them, built with g++ beside the tests like
// status_harness.cpp.  Returns the QPD_E_* code of a refusal, a positive qpd::ErrFlag
// for input the engine flags, else 0.
#include "qpd_list.hpp"

extern "C" int hl_decode_list(const qpd_config *c, const void *in, int32_t in_type, int64_t B, uint8_t *out,
                              const qpd_list_args *ls) {
    qpd_list::Req rq;
    std::string err;
    int fam = 0, dom = 0;
    const bool list = qpd_sched::family_of(c->kind, &fam, &dom) && (fam == QPD_SCL_LUT || fam == QPD_FASTSCL_LUT);
    const int rc = qpd_list::check(c->kind, list ? c->L : 1, c->crc_n, in_type, ls, &rq, err);
    if (rc) return rc;
    std::unique_ptr<qpd_host::Plan> p = qpd_host::make_plan(c);
    if (!p) return QPD_E_UNSUPPORTED;
    if (p->dom == qpd::DOM_LUT) {
        qpd_host::Engine<uint8_t> e(*p);
        if (in_type == QPD_IN_U8)
            return qpd_list::host_run(&e, (const uint8_t *)in, B, p->N, p->K, p->L, p->out_k, out, rq);
        return qpd_list::host_run(&e, (const int32_t *)in, B, p->N, p->K, p->L, p->out_k, out, rq);
    }
    qpd_host::Engine<double> e(*p);
    return qpd_list::host_run(&e, (const double *)in, B, p->N, p->K, p->L, p->out_k, out, rq);
}
