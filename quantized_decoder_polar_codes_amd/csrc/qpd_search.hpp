// qpd_search.hpp -- the argument rules of qpd_decode_search / _host (qpd.h), the mask set
// as the words the epilogues compare a path's CRC syndrome with (ca_winner_ranked,
// qpd_common.hpp; Engine::finish_search, qpd_host.hpp), and the host engine's search run.
// Host code without HIP, beside qpd_status.hpp and qpd_list.hpp, whose rules it extends:
// the CPU tests build it with the host engine (tests/native/search_harness.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "qpd.h"
#include "qpd_host.hpp"
#include "qpd_list.hpp"
#include "qpd_schedule.hpp"
#include "qpd_status.hpp"

namespace qpd_search {

// What one search call asks for, checked: the packed set and the outputs (device
// pointers in the device call, host pointers in the host call).
struct Req {
    bool on = false;              // a search call is being served
    std::vector<uint32_t> words;  // mask i's register value >> (crc_n - chk): what a syndrome is compared with
    uint32_t *syndrome = nullptr;  // [B][L]
    double *cand_metric = nullptr;  // [B][L]
    int32_t *hit_mask = nullptr;   // [B]
    int32_t *hit_rank = nullptr;   // [B]
    double *metric = nullptr;      // [B]
    bool any() const { return on; }
};

// The number of compared check bits (qpd_config.A): K - A for the LUT kinds, crc_n for
// the float CA-SCL.
inline int chk_bits(int kind, int K, int A, int crc_n) { return kind == QPD_CASCL_FLOAT ? crc_n : K - A; }

// kind, L, K, A, crc_n: the decoder's (qpd_config).  has_out: the call gave d_out / h_out.
// Returns QPD_OK or the refusal with its message in err; the input type and each mask
// row are qpd_stat::check's.
inline int check(int kind, int L, int K, int A, int crc_n, int32_t in_type, const qpd_search_args *sr, bool has_out,
                 Req *req, std::string &err) {
    auto refuse = [&](int rc, const char *msg) {
        err = msg;
        return rc;
    };
    *req = Req();
    if (!sr) return refuse(QPD_E_INVALID, "null qpd_search_args");
    int fam = 0, dom = 0;
    if (!qpd_sched::family_of(kind, &fam, &dom)) return refuse(QPD_E_INVALID, "bad kind");
    if (fam != QPD_SCL_LUT && fam != QPD_FASTSCL_LUT)
        return refuse(QPD_E_INVALID, "mask search: SC and FastSC decoders keep no list");
    if (!qpd_sched::is_ca(kind)) return refuse(QPD_E_INVALID, "mask search: not a CRC-aided decoder");
    if (sr->n_masks < 0 || sr->n_masks > QPD_MAX_SEARCH_MASKS)
        return refuse(QPD_E_INVALID, "n_masks must be in [0, QPD_MAX_SEARCH_MASKS]");
    const uint8_t zeros[32] = {0};  // crc_n <= 32
    qpd_status_args sa{};  // the input type and the width: the status call's rules, on an all-zero row
    sa.crc_mask_bits = sr->crc_mask_bits;
    sa.crc_mask = zeros;
    qpd_stat::Req one;
    const int rc = qpd_stat::check(kind, L, crc_n, in_type, &sa, &one, err);
    if (rc) return rc;
    const int bits = sr->crc_mask_bits;
    if (sr->n_masks > 0 && bits > 0 && !sr->crc_masks)
        return refuse(QPD_E_INVALID, "crc_masks is NULL with n_masks * crc_mask_bits > 0");
    // row i as qpd_stat::check packs one mask (bit l at register bit bits - 1 - l), then cut to
    // the compared bits: the low crc_n - chk register bits meet no check bit
    const int shift = crc_n - chk_bits(kind, K, A, crc_n);
    req->words.assign((size_t)sr->n_masks, 0u);
    for (int i = 0; i < sr->n_masks; ++i) {
        uint32_t m = 0;
        for (int l = 0; l < bits; ++l) {
            const uint8_t e = sr->crc_masks[(size_t)i * bits + l];
            if (e > 1) return refuse(QPD_E_INVALID, "crc_masks entries must be 0 or 1");
            m |= (uint32_t)e << (bits - 1 - l);
        }
        req->words[i] = shift >= 32 ? 0u : m >> shift;
    }
    if (sr->n_masks == 0 && (has_out || sr->hit_mask || sr->hit_rank || sr->metric))
        return refuse(QPD_E_INVALID, "n_masks == 0: no output path -- d_out, hit_mask, hit_rank and metric must be NULL");
    if (L == 1) return refuse(QPD_E_UNSUPPORTED, "mask search needs a list of at least 2 paths");
    if (L > qpd_list::kMaxListOut)
        return refuse(QPD_E_UNSUPPORTED, "mask search: L > 16 (the reference's argsort is the unstable introsort there)");
    req->on = true;
    req->syndrome = sr->cand_syndrome;
    req->cand_metric = sr->cand_metric;
    req->hit_mask = sr->hit_mask;
    req->hit_rank = sr->hit_rank;
    req->metric = sr->metric;
    return QPD_OK;
}

// B frames on the host engine with their search results (host pointers in rq; h_out may
// be NULL).  Returns the frames' error flags ORed (qpd::ErrFlag); a frame with a flag
// keeps what the caller left in its outputs.
template <class Eng, class In>
int host_run(Eng *eng, const In *h_in, int64_t B, int N, int L, int out_bits, uint8_t *h_out, const Req &rq) {
    int32_t flag = 0;
    eng->search.on = true;
    eng->search.words = rq.words.data();
    eng->search.n = (int)rq.words.size();
    for (int64_t b = 0; b < B; ++b) {
        eng->search.syndrome = rq.syndrome ? rq.syndrome + (size_t)b * L : nullptr;
        eng->search.metric = rq.cand_metric ? rq.cand_metric + (size_t)b * L : nullptr;
        eng->search.hit_mask = rq.hit_mask ? rq.hit_mask + b : nullptr;
        eng->search.hit_rank = rq.hit_rank ? rq.hit_rank + b : nullptr;
        const int f = eng->decode(h_in + b * N, h_out ? h_out + b * out_bits : nullptr);
        flag |= f;
        if (!f && rq.metric) rq.metric[b] = eng->last_metric;
    }
    eng->search = typename Eng::SearchOut();
    return flag;
}

}  // namespace qpd_search
