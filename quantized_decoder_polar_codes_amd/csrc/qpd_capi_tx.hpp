// qpd_capi_tx.hpp -- the transmit entry points' host code (qpd_encode,
// qpd_encode_host, qpd_tx_frames): the argument rules of qpd_tx.hpp applied to a
// handle, the channel's own rules (qpd_capi_mc.hpp), and the launches of
// qpd_tx.hip's kernels.  Host code.
#pragma once
#include <cstring>

#include "qpd_capi_mc.hpp"
#include "qpd_decoder.hpp"
#include "qpd_tx.hpp"
#include "qpd_tx_kernels.hpp"

namespace {

// The generator's argument block for this decoder's code (no channel yet).
int tx_code_block(qpd_decoder *d, qpd::McChannel *C) {
    if (!d->mc_pref.p) {
        const int rc = mc_constants(d);
        if (rc) return rc;
    }
    std::memset(C, 0, sizeof(*C));
    C->N = d->N;
    C->K = d->K;
    C->A = d->crc_n > 0 ? d->ca_A : d->K;
    C->crc_n = d->crc_n;
    C->info_mask = (const uint32_t *)d->info_mask.p;
    C->info_pref = (const int32_t *)d->mc_pref.p;
    C->crc_tab = (const uint32_t *)d->mc_crc.p;
    return QPD_OK;
}

// One resident round of one-wave workgroups, grid-stride over the frames (mc_launch).
int tx_grid(const void *kfn, size_t lds, int64_t B) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kfn, 64, lds) != hipSuccess || per_cu <= 0) per_cu = 8;
    return (int)std::min<int64_t>(B, (int64_t)device_cus() * per_cu);
}

// qpd_encode's launch on stream st.  Caller: lock held, stream ordered.
int tx_encode_launch(qpd_decoder *d, const uint8_t *d_msg, int64_t B, uint32_t mask, uint8_t *d_info, uint8_t *d_cw,
                     hipStream_t st) {
    qpd::McChannel C;
    const int rc = tx_code_block(d, &C);
    if (rc) return rc;
    qpd::TxIo io{d_msg, d_info, d_cw, nullptr, (int32_t *)d->err.p, mask, 0};
    const void *kfn = qpd::tx_encode_kernel_fn();
    const size_t lds = qpd::mc_lds_bytes(d->N, d->K, qpd::MC_LLR);  // the bit words alone
    const int grid = tx_grid(kfn, lds, B);
    void *args[] = {&C, &B, &io};
    return timed_launch(d, QPD_KC_MC, st, [&]() -> int {
        QPD_HIP(hipLaunchKernel(kfn, dim3(grid), dim3(64), args, lds, st));
        QPD_HIP(hipGetLastError());
        return QPD_OK;
    });
}

// qpd_tx_frames' launch on stream st (mc_launch with the message given).
int tx_frames_launch(qpd_decoder *d, const qpd_mc_channel *ch, const double *rec, uint64_t seed, int64_t frame0, int64_t B,
                     const uint8_t *d_msg, uint32_t mask, int no_signal, int32_t out_type, void *d_frames, hipStream_t st) {
    const int out = out_type == QPD_TX_LLR_F64 ? (rec ? qpd::TX_LLR_REC : qpd::TX_LLR) : out_type;
    qpd::McChannel C;
    int rc = tx_code_block(d, &C);
    if (rc) return rc;
    if (out == qpd::TX_LLR_REC && (rc = mc_rec_table(d, rec, ch->q, st))) return rc;
    C.q = ch->q;
    C.seed_lo = (uint32_t)seed;
    C.seed_hi = (uint32_t)(seed >> 32);
    C.sigma = ch->sigma;
    C.inv_s2 = 1.0 / (ch->sigma * ch->sigma);  // the driver's sigma ** 2, inverted once (mc_launch)
    if (out == qpd::TX_LLR_REC) C.rec = (const double *)d->mc_rec.p;
    if (out != qpd::TX_LLR) {
        C.n_edges = ch->n_edges;
        for (int i = 0; i < ch->n_edges; ++i) C.edges[i] = ch->edges[i];
        for (int i = 0; i + 1 < ch->n_edges; ++i) C.lut[i] = ch->lut[i];
    }
    qpd::TxIo io{d_msg, nullptr, nullptr, d_frames, (int32_t *)d->err.p, mask, no_signal};
    const void *kfn = qpd::tx_frames_kernel_fn(out);
    const size_t lds = qpd::mc_lds_bytes(d->N, d->K, out == qpd::TX_LLR ? qpd::MC_LLR
                                                     : out == qpd::TX_LLR_REC ? qpd::MC_LLR_REC : qpd::MC_SYM);
    const int grid = tx_grid(kfn, lds, B);
    void *args[] = {&C, &frame0, &B, &io};
    return timed_launch(d, QPD_KC_MC, st, [&]() -> int {
        QPD_HIP(hipLaunchKernel(kfn, dim3(grid), dim3(64), args, lds, st));
        QPD_HIP(hipGetLastError());
        return QPD_OK;
    });
}

// The encoder's host constants, built once per handle (the information mask is
// read back from the device copy qpd_create made).  Caller: lock held.
int tx_host_code(qpd_decoder *d) {
    if (d->tx_code) return QPD_OK;
    int rc = set_device(d);
    if (rc) return rc;
    const int nw = (d->N + 31) / 32;
    std::vector<uint32_t> mask(nw, 0u);
    QPD_HIP(hipMemcpyAsync(mask.data(), d->info_mask.p, nw * sizeof(uint32_t), hipMemcpyDeviceToHost, d->hs));
    QPD_HIP(hipStreamSynchronize(d->hs));
    d->tx_code.reset(new qpd_tx::Code(qpd_tx::make_code(d->N, d->K, d->ca_A, d->crc_n, d->crc_q, mask.data())));
    return QPD_OK;
}

}  // namespace
