// Test harness (CPU): qpd_decode_status_host's host-engine branch without a
// device -- the argument rules (qpd_status.hpp: check) and the host engine's
// status run (host_run) exactly as qpd_capi.hip calls them, built with g++ beside
// the tests like host_engine_harness.cpp.  Returns the QPD_E_* code of a refusal,
// a positive qpd::ErrFlag for input the engine flags, else 0.
#include "qpd_status.hpp"

extern "C" int hs_decode_status(const qpd_config *c, const void *in, int32_t in_type, int64_t B, uint8_t *out,
                                const qpd_status_args *st) {
    qpd_stat::Req rq;
    std::string err;
    const int rc = qpd_stat::check(c->kind, c->L, c->crc_n, in_type, st, &rq, err);
    if (rc) return rc;
    std::unique_ptr<qpd_host::Plan> p = qpd_host::make_plan(c);
    if (!p) return QPD_E_UNSUPPORTED;
    if (p->dom == qpd::DOM_LUT) {
        qpd_host::Engine<uint8_t> e(*p);
        if (in_type == QPD_IN_U8) return qpd_stat::host_run(&e, (const uint8_t *)in, B, p->N, p->out_k, out, rq);
        return qpd_stat::host_run(&e, (const int32_t *)in, B, p->N, p->out_k, out, rq);
    }
    qpd_host::Engine<double> e(*p);
    return qpd_stat::host_run(&e, (const double *)in, B, p->N, p->out_k, out, rq);
}
