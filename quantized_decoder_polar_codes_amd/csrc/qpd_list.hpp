// qpd_list.hpp -- the argument rules of qpd_decode_list / _host (qpd.h) and the host
// engine's list run.  Host code without HIP, beside qpd_status.hpp, whose rules it
// extends: the CPU tests build it with the host engine (tests/native/list_harness.cpp).
#pragma once
#include <cstdint>
#include <string>

#include "qpd.h"
#include "qpd_host.hpp"
#include "qpd_schedule.hpp"
#include "qpd_status.hpp"

namespace qpd_list {

// Candidates are reported in the reference's argsort(PML) order, which is the stable
// order only while libstdc++ sorts by insertion (L <= 16, stl_sort.hpp kThreshold).
constexpr int kMaxListOut = 16;

// What one list call asks for, checked: the mask word and the outputs (device
// pointers in the device call, host pointers in the host call).
struct Req {
    uint32_t mask = 0;
    uint8_t *bits = nullptr;    // [B][L][K]
    double *metric = nullptr;   // [B][L]
    uint8_t *pass = nullptr;    // [B][L]
    int32_t *chosen = nullptr;  // [B]
    bool any() const { return bits != nullptr; }
};

// kind, L, crc_n: the decoder's (qpd_config).  Returns QPD_OK or the refusal with its
// message in err; everything the list call shares with the status call (the input
// type, the mask) is qpd_stat::check's.
inline int check(int kind, int L, int crc_n, int32_t in_type, const qpd_list_args *ls, Req *req, std::string &err) {
    auto refuse = [&](int rc, const char *msg) {
        err = msg;
        return rc;
    };
    *req = Req();
    if (!ls) return refuse(QPD_E_INVALID, "null qpd_list_args");
    int fam = 0, dom = 0;
    if (!qpd_sched::family_of(kind, &fam, &dom)) return refuse(QPD_E_INVALID, "bad kind");
    if (fam != QPD_SCL_LUT && fam != QPD_FASTSCL_LUT)
        return refuse(QPD_E_INVALID, "list output: SC and FastSC decoders keep no list");
    if (ls->cand_pass && !qpd_sched::is_ca(kind)) return refuse(QPD_E_INVALID, "cand_pass: not a CRC-aided decoder");
    qpd_status_args sa{};  // the input type and the mask: the status call's rules
    sa.crc_mask = ls->crc_mask;
    sa.crc_mask_bits = ls->crc_mask_bits;
    qpd_stat::Req sr;
    const int rc = qpd_stat::check(kind, L, crc_n, in_type, &sa, &sr, err);
    if (rc) return rc;
    if (!ls->cand_bits) return refuse(QPD_E_INVALID, "cand_bits is NULL");
    if (L == 1) return refuse(QPD_E_UNSUPPORTED, "list output needs a list of at least 2 paths");
    if (L > kMaxListOut)
        return refuse(QPD_E_UNSUPPORTED, "list output: L > 16 (the reference's argsort is the unstable introsort there)");
    req->mask = sr.mask;
    req->bits = ls->cand_bits;
    req->metric = ls->cand_metric;
    req->pass = ls->cand_pass;
    req->chosen = ls->chosen;
    return QPD_OK;
}

// B frames on the host engine with their lists (host pointers in rq; h_out may be
// NULL).  Returns the frames' error flags ORed (qpd::ErrFlag); a frame with a flag
// keeps what the caller left in its outputs.
template <class Eng, class In>
int host_run(Eng *eng, const In *h_in, int64_t B, int N, int K, int L, int out_bits, uint8_t *h_out, const Req &rq) {
    int32_t flag = 0;
    eng->crc_mask = rq.mask;
    for (int64_t b = 0; b < B; ++b) {
        eng->list.bits = rq.bits + (size_t)b * L * K;
        eng->list.metric = rq.metric ? rq.metric + (size_t)b * L : nullptr;
        eng->list.pass = rq.pass ? rq.pass + (size_t)b * L : nullptr;
        eng->list.chosen = rq.chosen ? rq.chosen + b : nullptr;
        flag |= eng->decode(h_in + b * N, h_out ? h_out + b * out_bits : nullptr);
    }
    eng->list = typename Eng::ListOut();
    eng->crc_mask = 0;
    return flag;
}

}  // namespace qpd_list
