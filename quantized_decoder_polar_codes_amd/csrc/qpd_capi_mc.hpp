// qpd_capi_mc.hpp -- the Monte-Carlo entry points' host code: the channel
// check, the frame generator's launch (qpd_mc.hip), and generate + decode +
// count chunk by chunk.  Host code.
#pragma once
#include <cstring>

#include "qpd_capi_decode.hpp"
#include "qpd_decoder.hpp"
#include "qpd_mc.hip"

namespace {

int check_channel(const qpd_mc_channel *ch) {
    if (ch->n_edges < 2 || ch->n_edges > qpd::kMcMaxEdges) return fail(QPD_E_INVALID, "n_edges must be in [2, 257]");
    if (!ch->edges || !ch->lut) return fail(QPD_E_INVALID, "null channel quantizer");
    if (!(ch->sigma > 0) || ch->q < 2) return fail(QPD_E_INVALID, "sigma must be > 0 and q >= 2");
    for (int i = 0; i + 1 < ch->n_edges; ++i) {
        if (!(ch->edges[i] <= ch->edges[i + 1])) return fail(QPD_E_INVALID, "edges must be ascending");
        if (ch->lut[i] < 0 || ch->lut[i] >= ch->q) return fail(QPD_E_INVALID, "lut entry outside [0, q)");
    }
    return QPD_OK;
}

// The checks the two Monte-Carlo entry points share.  *run = false where there
// is nothing to launch (a refusal, or an empty range: QPD_OK).  lut_only: the
// entry point decodes too (qpd_mc_decode), so it needs a LUT decoder.
int check_mc_args(const qpd_decoder *d, const qpd_mc_channel *ch, bool lut_only, int64_t frame0, int64_t B, const void *d_msg,
                  const void *d_buf, bool *run) {
    *run = false;
    if (!d || !ch) return fail(QPD_E_INVALID, "null argument");
    if (lut_only && d->dom != qpd::DOM_LUT)
        return fail(QPD_E_INVALID, "qpd_mc_decode needs a LUT decoder (int32 channel symbols)");
    if (B < 0 || frame0 < 0) return fail(QPD_E_INVALID, "negative frame range");
    if (B == 0) return QPD_OK;
    if (!d_msg || !d_buf) return fail(QPD_E_INVALID, "null buffer");
    const int rc = check_channel(ch);
    *run = !rc;
    return rc;
}

// Per-decoder constants of the generator, built at the first call: the info
// bits before each word of the mask, and the CRC contribution per message bit.
int mc_constants(qpd_decoder *d) {
    const int nw = (d->N + 31) / 32;
    std::vector<int32_t> pref(nw, 0);
    std::vector<uint32_t> mask(nw, 0u);
    QPD_HIP(hipMemcpyAsync(mask.data(), d->info_mask.p, nw * sizeof(uint32_t), hipMemcpyDeviceToHost, d->hs));
    QPD_HIP(hipStreamSynchronize(d->hs));
    for (int w = 1; w < nw; ++w) pref[w] = pref[w - 1] + __builtin_popcount(mask[w - 1]);
    // CRC register after message bit j and A-1-j zero bits (the register is
    // linear in the message bits, utils.cpp:77-92): tab[A-1] = taps,
    // tab[j] = one zero step of tab[j+1]
    const int A = d->crc_n > 0 ? d->ca_A : 0;
    std::vector<uint32_t> tab(std::max(A, 1), 0u);
    if (A > 0) {
        const uint32_t top = 1u << (d->crc_n - 1), msk = (top << 1) - 1u;
        tab[A - 1] = d->crc_q & msk;
        for (int j = A - 2; j >= 0; --j) {
            const uint32_t r = tab[j + 1];
            tab[j] = ((r << 1) & msk) ^ ((r & top) ? d->crc_q : 0u);
        }
    }
    const int rc = upload(d->mc_pref, pref.data(), pref.size(), d->hs);
    return rc ? rc : upload(d->mc_crc, tab.data(), tab.size(), d->hs);
}

// The Monte-Carlo generator on stream st: int32 symbols to `rows`, or (pre)
// the decoder's root pre-pass rows.  Caller: lock held, stream ordered.
int mc_launch(qpd_decoder *d, const qpd_mc_channel *ch, uint64_t seed, int64_t frame0, int64_t B, uint8_t *d_msg,
              int32_t *rows, bool pre, hipStream_t st) {
    if (!d->mc_pref.p) {
        const int rc = mc_constants(d);
        if (rc) return rc;
    }
    qpd::McChannel C;
    std::memset(&C, 0, sizeof(C));
    C.N = d->N;
    C.K = d->K;
    C.A = d->crc_n > 0 ? d->ca_A : d->K;
    C.crc_n = d->crc_n;
    C.q = ch->q;
    C.n_edges = ch->n_edges;
    C.seed_lo = (uint32_t)seed;
    C.seed_hi = (uint32_t)(seed >> 32);
    C.sigma = ch->sigma;
    C.inv_s2 = 1.0 / (ch->sigma * ch->sigma);  // the driver's sigma ** 2, inverted once
    C.info_mask = (const uint32_t *)d->info_mask.p;
    C.info_pref = (const int32_t *)d->mc_pref.p;
    C.crc_tab = (const uint32_t *)d->mc_crc.p;
    C.f_tab = d->fplan.f_tab;
    C.g_tab = d->fplan.g_tab;
    for (int i = 0; i < ch->n_edges; ++i) C.edges[i] = ch->edges[i];
    for (int i = 0; i + 1 < ch->n_edges; ++i) C.lut[i] = ch->lut[i];
    int per_cu = 0;
    const int ncu = device_cus();
    const size_t lds = qpd::mc_lds_bytes(d->N, d->K, pre);
    // one resident round of workgroups (grid-stride over frames): a grid
    // larger than what fits at once runs its last workgroups as a tail
    const void *kfn = pre ? reinterpret_cast<const void *>(&qpd::mc_frames_kernel<true>)
                          : reinterpret_cast<const void *>(&qpd::mc_frames_kernel<false>);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kfn, 64, lds) != hipSuccess || per_cu <= 0) per_cu = 8;
    const int grid = (int)std::min<int64_t>(B, (int64_t)ncu * per_cu);
    return timed_launch(d, QPD_KC_MC, st, [&]() -> int {
        if (pre)
            hipLaunchKernelGGL(qpd::mc_frames_kernel<true>, dim3(grid), dim3(64), lds, st, C, frame0, B, d_msg, rows);
        else
            hipLaunchKernelGGL(qpd::mc_frames_kernel<false>, dim3(grid), dim3(64), lds, st, C, frame0, B, d_msg, rows);
        QPD_HIP(hipGetLastError());
        return QPD_OK;
    });
}

// qpd_mc_decode's work on stream st (caller: lock held, stream ordered):
// frames generated, decoded and, with d_counts, counted, chunk by chunk.
int mc_decode(qpd_decoder *d, const qpd_mc_channel *ch, uint64_t seed, int64_t frame0, int64_t B, uint8_t *d_msg,
              uint8_t *d_out, int64_t *d_counts, hipStream_t st) {
    // fused: the generator writes the root pre-pass rows the decode
    // kernel reads (fast engine in pre-mode; symbols < q <= v need no
    // range check); else int32 symbols in a buffer of its own
    const bool fused = d->engine == QPD_ENGINE_FAST && d->pre && ch->q <= d->v;
    d->last_engine = QPD_RAN_GPU;
    d->u8_staged = 0;
    int rc = QPD_OK;
    const int64_t chunk = fused ? reserve_pre_rows(d, B, &rc)
                                : reserve_symbols(d, d->mc_sym, B, 0, "Monte-Carlo symbols hipMalloc: ", &rc);
    if (rc) return rc;
    void *buf = fused ? d->pre_rows.p : d->mc_sym.p;
    for (int64_t f0 = 0; f0 < B; f0 += chunk) {
        const int64_t Bc = std::min<int64_t>(chunk, B - f0);
        int r = mc_launch(d, ch, seed, frame0 + f0, Bc, d_msg + f0 * d->out_bits, (int32_t *)buf, fused, st);
        if (r) return r;
        uint8_t *out = d_out + f0 * d->out_bits;
        r = fused ? decode_pre_rows(d, (const uint32_t *)buf, Bc, out, st)
                  : decode_impl(d, (const int32_t *)buf, Bc, out, st);
        if (r) return r;
    }
    if (d_counts) {  // the driver's error counters over the whole range
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((B + 3) / 4, (int64_t)device_cus() * 8));
        hipLaunchKernelGGL(qpd::mc_count_kernel, dim3(grid), dim3(256), 0, st, d_out, d_msg, B, d->out_bits,
                           (unsigned long long *)d_counts);
        QPD_HIP(hipGetLastError());
    }
    return QPD_OK;
}

}  // namespace
