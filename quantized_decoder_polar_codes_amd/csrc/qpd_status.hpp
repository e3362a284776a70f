// qpd_status.hpp -- the argument rules of qpd_decode_status / _host (qpd.h) and
// the CRC mask as the register word the epilogues XOR (ca_winner, qpd_common.hpp;
// Engine::finish, qpd_host.hpp), plus the host engine's status run.  Host code
// without HIP: the CPU tests build it beside the host engine
// (tests/native/status_harness.cpp).
#pragma once
#include <cstdint>
#include <string>

#include "qpd.h"
#include "qpd_host.hpp"
#include "qpd_schedule.hpp"

namespace qpd_stat {

// What one status call asks for, checked: the mask word and the two outputs
// (device pointers in the device call, host pointers in the host call).
struct Req {
    uint32_t mask = 0;
    double *metric = nullptr;
    uint8_t *pass = nullptr;
    bool any() const { return mask || metric || pass; }
};

// kind, L, crc_n: the decoder's (qpd_config).  st may be NULL (nothing asked).
// Returns QPD_OK or the refusal with its message in err.
inline int check(int kind, int L, int crc_n, int32_t in_type, const qpd_status_args *st, Req *req, std::string &err) {
    auto refuse = [&](int rc, const char *msg) {
        err = msg;
        return rc;
    };
    int fam = 0, dom = 0;
    if (!qpd_sched::family_of(kind, &fam, &dom)) return refuse(QPD_E_INVALID, "bad kind");
    if (in_type < QPD_IN_I32 || in_type > QPD_IN_F64) return refuse(QPD_E_INVALID, "in_type must be QPD_IN_I32, _U8 or _F64");
    if ((in_type == QPD_IN_F64) != (dom != qpd::DOM_LUT))
        return refuse(QPD_E_INVALID, dom == qpd::DOM_LUT ? "LUT decoders take channel symbols: in_type QPD_IN_I32 or QPD_IN_U8"
                                                         : "this decoder takes float64 LLRs: in_type QPD_IN_F64");
    *req = Req();
    if (!st) return QPD_OK;
    const bool list = fam == QPD_SCL_LUT || fam == QPD_FASTSCL_LUT;
    const bool ca = qpd_sched::is_ca(kind);
    if (st->metric && !list) return refuse(QPD_E_INVALID, "metric: SC and FastSC decoders have no path metric");
    if (st->crc_pass && !ca) return refuse(QPD_E_INVALID, "crc_pass: not a CRC-aided decoder");
    // (the reference writes out of bounds for an RNTI longer than the CRC, CASCLWithRNTI.cpp:222-224)
    if (st->crc_mask_bits < 0 || st->crc_mask_bits > (ca ? crc_n : 0))
        return refuse(QPD_E_INVALID, ca ? "crc_mask_bits must be in [0, crc_n]" : "crc_mask: not a CRC-aided decoder");
    if (st->crc_mask_bits > 0 && !st->crc_mask) return refuse(QPD_E_INVALID, "crc_mask is NULL with crc_mask_bits > 0");
    // mask bit l meets check-code bit crc_n - bits + l, register bit bits - 1 - l
    for (int l = 0; l < st->crc_mask_bits; ++l) {
        if (st->crc_mask[l] > 1) return refuse(QPD_E_INVALID, "crc_mask entries must be 0 or 1");
        req->mask |= (uint32_t)st->crc_mask[l] << (st->crc_mask_bits - 1 - l);
    }
    if ((st->metric || st->crc_pass) && list && L == 1)
        return refuse(QPD_E_UNSUPPORTED, "decode status needs a list of at least 2 paths");
    req->metric = st->metric;
    req->pass = st->crc_pass;
    return QPD_OK;
}

// B frames on the host engine with their status (host pointers in rq).  Returns
// the frames' error flags ORed (qpd::ErrFlag).
template <class Eng, class In>
int host_run(Eng *eng, const In *h_in, int64_t B, int N, int out_bits, uint8_t *h_out, const Req &rq) {
    int32_t flag = 0;
    eng->crc_mask = rq.mask;
    for (int64_t b = 0; b < B; ++b) {
        const int f = eng->decode(h_in + b * N, h_out + b * out_bits);
        flag |= f;
        if (f) continue;  // nothing decoded: the frame's status stays as the caller left it
        if (rq.metric) rq.metric[b] = eng->last_metric;
        if (rq.pass) rq.pass[b] = (uint8_t)eng->last_pass;
    }
    eng->crc_mask = 0;
    return flag;
}

}  // namespace qpd_stat
