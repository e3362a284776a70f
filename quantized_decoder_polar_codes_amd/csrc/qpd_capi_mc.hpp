// qpd_capi_mc.hpp -- the Monte-Carlo entry points' host code: the channel
// check, the frame generator's launch (qpd_mc.hip), and generate + decode +
// count chunk by chunk.  Host code.
#pragma once
#include <cmath>
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

// d_msg's alignment (include/qpd.h): rows of a multiple of 8 message bits are
// stored 8 bytes at a time (mc_frames_kernel), so their base is 8-byte aligned.
int check_msg_alignment(const qpd_decoder *d, const void *d_msg) {
    if ((d->out_bits & 7) == 0 && ((uintptr_t)d_msg & 7u) != 0)
        return fail(QPD_E_INVALID, "d_msg alignment: rows of a multiple of 8 message bits need an 8-byte aligned base");
    return QPD_OK;
}

// The LLR entry points' channel.  Without rec the quantizer is unused (edges /
// lut may be null, n_edges 0): only sigma counts.  With rec: a whole channel
// quantizer, and one finite reconstruction value per symbol (the generator
// stages up to 256 of them).
int check_llr_channel(const qpd_mc_channel *ch, const double *rec) {
    if (!rec) return ch->sigma > 0 ? QPD_OK : fail(QPD_E_INVALID, "sigma must be > 0");
    const int rc = check_channel(ch);
    if (rc) return rc;
    if (ch->q > qpd::kMcMaxEdges - 1) return fail(QPD_E_INVALID, "rec: q must be at most 256");
    for (int i = 0; i < ch->q; ++i)
        if (!std::isfinite(rec[i])) return fail(QPD_E_INVALID, "rec entries must be finite");
    return QPD_OK;
}

// The checks the two LLR entry points share (as check_mc_args).  f64_only: the
// entry point decodes too (qpd_mc_decode_f64), so it needs a float64-LLR decoder.
int check_mc_llr_args(const qpd_decoder *d, const qpd_mc_channel *ch, const double *rec, bool f64_only, int64_t frame0,
                      int64_t B, const void *d_msg, const void *d_buf, bool *run) {
    *run = false;
    if (!d || !ch) return fail(QPD_E_INVALID, "null argument");
    if (f64_only && d->dom == qpd::DOM_LUT)
        return fail(QPD_E_INVALID, "qpd_mc_decode_f64 needs a float64-LLR decoder: use qpd_mc_decode");
    // the generator appends K - A bits of the crc_n-bit CRC; QPD_CASCL_FLOAT compares
    // exactly crc_n, so it is served where A + crc_n == K (the driver's own case)
    if (d->crc_n > 0 && d->K - d->ca_A > d->crc_n)
        return fail(QPD_E_UNSUPPORTED, "Monte-Carlo frames of a CRC-aided decoder need K - A <= crc_n (CASCLDecoder: A + crc_n == K)");
    if (B < 0 || frame0 < 0) return fail(QPD_E_INVALID, "negative frame range");
    if (B == 0) return QPD_OK;
    if (!d_msg || !d_buf) return fail(QPD_E_INVALID, "null buffer");
    if (check_msg_alignment(d, d_msg)) return QPD_E_INVALID;
    const int rc = check_llr_channel(ch, rec);
    *run = !rc;
    return rc;
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
    if (check_msg_alignment(d, d_msg)) return QPD_E_INVALID;
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

// The device copy of the reconstruction table (MC_LLR_REC), uploaded on stream
// st when it differs from the last call's, complete on return: the caller's
// array is not read after the call, and launches queued earlier (st is ordered
// after them) have read the previous table.
int mc_rec_table(qpd_decoder *d, const double *rec, int q, hipStream_t st) {
    if (!d->mc_rec.p) QPD_HIP(hipMalloc(&d->mc_rec.p, (qpd::kMcMaxEdges - 1) * sizeof(double)));
    if ((int)d->mc_rec_host.size() == q && std::equal(rec, rec + q, d->mc_rec_host.begin(), [](double a, double b) {
            return std::memcmp(&a, &b, sizeof a) == 0;
        }))
        return QPD_OK;
    d->mc_rec_host.clear();  // no table on the device until the copy below is complete
    QPD_HIP(hipMemcpyAsync(d->mc_rec.p, rec, q * sizeof(double), hipMemcpyHostToDevice, st));
    QPD_HIP(hipStreamSynchronize(st));
    d->mc_rec_host.assign(rec, rec + q);
    return QPD_OK;
}

const void *mc_kernel(int mode) {
    switch (mode) {
        case qpd::MC_SYM: return reinterpret_cast<const void *>(&qpd::mc_frames_kernel<qpd::MC_SYM>);
        case qpd::MC_PRE: return reinterpret_cast<const void *>(&qpd::mc_frames_kernel<qpd::MC_PRE>);
        case qpd::MC_PRE_LO: return reinterpret_cast<const void *>(&qpd::mc_frames_kernel<qpd::MC_PRE_LO>);
        case qpd::MC_LLR: return reinterpret_cast<const void *>(&qpd::mc_frames_kernel<qpd::MC_LLR>);
        default: return reinterpret_cast<const void *>(&qpd::mc_frames_kernel<qpd::MC_LLR_REC>);
    }
}

// The Monte-Carlo generator on stream st, `rows` by mode (qpd::McMode): int32
// symbols, the decoder's root pre-pass rows, or float64 LLRs (rec: null, or the
// host table of MC_LLR_REC).  Caller: lock held, stream ordered.
int mc_launch(qpd_decoder *d, const qpd_mc_channel *ch, uint64_t seed, int64_t frame0, int64_t B, uint8_t *d_msg,
              void *rows, int mode, hipStream_t st, const double *rec = nullptr) {
    if (!d->mc_pref.p) {
        const int rc = mc_constants(d);
        if (rc) return rc;
    }
    if (mode == qpd::MC_LLR_REC) {
        const int rc = mc_rec_table(d, rec, ch->q, st);
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
    if (mode == qpd::MC_LLR_REC) C.rec = (const double *)d->mc_rec.p;  // in f_tab's place (McChannel)
    if (mode != qpd::MC_LLR) {  // MC_LLR: no quantizer (the channel's may be absent)
        for (int i = 0; i < ch->n_edges; ++i) C.edges[i] = ch->edges[i];
        for (int i = 0; i + 1 < ch->n_edges; ++i) C.lut[i] = ch->lut[i];
    } else {
        C.n_edges = 0;
    }
    int per_cu = 0;
    const int ncu = device_cus();
    const size_t lds = qpd::mc_lds_bytes(d->N, d->K, mode);
    // one resident round of workgroups (grid-stride over frames): a grid
    // larger than what fits at once runs its last workgroups as a tail
    const void *kfn = mc_kernel(mode);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kfn, 64, lds) != hipSuccess || per_cu <= 0) per_cu = 8;
    const int grid = (int)std::min<int64_t>(B, (int64_t)ncu * per_cu);
    void *args[] = {&C, &frame0, &B, &d_msg, &rows};
    return timed_launch(d, QPD_KC_MC, st, [&]() -> int {
        QPD_HIP(hipLaunchKernel(kfn, dim3(grid), dim3(64), args, lds, st));
        QPD_HIP(hipGetLastError());
        return QPD_OK;
    });
}

// Bit and block errors of B decoded frames against their messages, added to d_counts.
int mc_count(qpd_decoder *d, const uint8_t *d_out, const uint8_t *d_msg, int64_t B, int64_t *d_counts, hipStream_t st) {
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((B + 3) / 4, (int64_t)device_cus() * 8));
    hipLaunchKernelGGL(qpd::mc_count_kernel, dim3(grid), dim3(256), 0, st, d_out, d_msg, B, d->out_bits,
                       (unsigned long long *)d_counts);
    QPD_HIP(hipGetLastError());
    return QPD_OK;
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
        int r = mc_launch(d, ch, seed, frame0 + f0, Bc, d_msg + f0 * d->out_bits, buf, fused ? (d->row_lo ? qpd::MC_PRE_LO : qpd::MC_PRE) : qpd::MC_SYM, st);
        if (r) return r;
        uint8_t *out = d_out + f0 * d->out_bits;
        r = fused ? decode_pre_rows(d, (const uint32_t *)buf, Bc, out, st)
                  : decode_impl(d, (const int32_t *)buf, Bc, out, st);
        if (r) return r;
    }
    // the driver's error counters over the whole range
    return d_counts ? mc_count(d, d_out, d_msg, B, d_counts, st) : QPD_OK;
}

// qpd_mc_decode_f64's work on stream st (caller: lock held, stream ordered):
// a chunk of LLRs generated into the decoder's own buffer (mc_llr_chunk_frames,
// qpd_chunk.hpp; fewer after an allocation failure), decoded, and so on; then
// the counters over the whole range.
int mc_decode_f64(qpd_decoder *d, const qpd_mc_channel *ch, const double *rec, uint64_t seed, int64_t frame0, int64_t B,
                  uint8_t *d_msg, uint8_t *d_out, int64_t *d_counts, hipStream_t st) {
    int rc = QPD_OK;
    const int64_t chunk = d->mc_llr.reserve(std::min<int64_t>(B, qpd::mc_llr_chunk_frames(d->N)), (size_t)d->N * sizeof(double),
                                            "Monte-Carlo LLRs hipMalloc: ", &rc);
    if (rc) return rc;
    double *buf = (double *)d->mc_llr.p;
    for (int64_t f0 = 0; f0 < B; f0 += chunk) {
        const int64_t Bc = std::min<int64_t>(chunk, B - f0);
        if ((rc = mc_launch(d, ch, seed, frame0 + f0, Bc, d_msg + f0 * d->out_bits, buf, rec ? qpd::MC_LLR_REC : qpd::MC_LLR,
                            st, rec)))
            return rc;
        if ((rc = decode_f64_impl(d, buf, Bc, d_out + f0 * d->out_bits, st))) return rc;
    }
    return d_counts ? mc_count(d, d_out, d_msg, B, d_counts, st) : QPD_OK;
}

}  // namespace
