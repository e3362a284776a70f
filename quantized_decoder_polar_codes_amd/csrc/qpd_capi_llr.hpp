// qpd_capi_llr.hpp -- the LLR entry points' host code (qpd_quantize_llr,
// qpd_decode_llr, qpd_decode_llr_host): the quantizer's check, the front
// kernel's launch (qpd_llr.hip), quantize + decode chunk by chunk, and the
// host-buffer call's quantizer.  Host code.
#pragma once
#include <cstring>
#include <vector>

#include "qpd_capi_decode.hpp"
#include "qpd_capi_host.hpp"
#include "qpd_decoder.hpp"
#include "qpd_llr.hip"

namespace {

// The channel quantizer of the LLR entry points: qpd_mc_channel without its
// sigma, which nothing here reads (check_channel, qpd_capi_mc.hpp, wants one).
int check_quantizer(const qpd_mc_channel *ch) {
    if (ch->n_edges < 2 || ch->n_edges > qpd::kLlrMaxEdges) return fail(QPD_E_INVALID, "n_edges must be in [2, 257]");
    if (!ch->edges || !ch->lut) return fail(QPD_E_INVALID, "null channel quantizer");
    if (ch->q < 2) return fail(QPD_E_INVALID, "q must be >= 2");
    for (int i = 0; i + 1 < ch->n_edges; ++i) {
        if (!(ch->edges[i] <= ch->edges[i + 1])) return fail(QPD_E_INVALID, "edges must be ascending");
        if (ch->lut[i] < 0 || ch->lut[i] >= ch->q) return fail(QPD_E_INVALID, "lut entry outside [0, q)");
    }
    return QPD_OK;
}

size_t llr_size(int32_t type) { return type == QPD_LLR_F32 ? sizeof(float) : sizeof(double); }

// The checks the three LLR entry points share.  *run = false where there is
// nothing to do (a refusal, or an empty batch: QPD_OK).  q_max: the largest q the
// entry point serves (the decoder's v, or 256 symbols of a byte).
int check_llr_args(const qpd_decoder *d, const qpd_mc_channel *ch, const void *llr, int32_t type, int64_t B,
                   const void *out, int q_max, const char *q_what, bool *run) {
    *run = false;
    if (!d || !ch) return fail(QPD_E_INVALID, "null argument");
    if (d->dom != qpd::DOM_LUT)
        return fail(QPD_E_INVALID, "this decoder takes float64 LLRs as they are: use qpd_decode_f64");
    if (type != QPD_LLR_F64 && type != QPD_LLR_F32) return fail(QPD_E_INVALID, "llr_type must be QPD_LLR_F64 or QPD_LLR_F32");
    if (B < 0) return fail(QPD_E_INVALID, "negative batch");
    if (B == 0) return QPD_OK;
    if (!llr || !out) return fail(QPD_E_INVALID, "null buffer");
    if ((uintptr_t)llr % llr_size(type)) return fail(QPD_E_INVALID, "the LLRs need 8-byte (float64) / 4-byte (float32) alignment");
    const int rc = check_quantizer(ch);
    if (rc) return rc;
    if (ch->q > (q_max < 0 ? d->v : q_max)) return fail(QPD_E_INVALID, q_what);
    *run = true;
    return QPD_OK;
}

// The front kernel's arguments that do not change from chunk to chunk.
qpd::LlrFront llr_front_args(const qpd_decoder *d, const qpd_mc_channel *ch) {
    qpd::LlrFront C;
    std::memset(&C, 0, sizeof(C));
    C.Q = qpd::llr_quant_params(ch->edges, ch->n_edges, ch->q);
    C.N = d->N;
    C.n = d->n;
    C.f_tab = d->fplan.f_tab;
    C.g_tab = d->fplan.g_tab;
    C.err = (int32_t *)d->err.p;
    for (int i = 0; i < ch->n_edges; ++i) C.edges[i] = ch->edges[i];
    for (int i = 0; i + 1 < ch->n_edges; ++i) C.lut[i] = (uint8_t)ch->lut[i];
    return C;
}

template <class T>
const void *llr_kernel(int form, bool coop) {
    switch (form) {
        case qpd::LLR_PRE:
            return coop ? reinterpret_cast<const void *>(&qpd::llr_front_kernel<T, qpd::LLR_PRE, true>)
                        : reinterpret_cast<const void *>(&qpd::llr_front_kernel<T, qpd::LLR_PRE, false>);
        case qpd::LLR_PRE_LO:
            return coop ? reinterpret_cast<const void *>(&qpd::llr_front_kernel<T, qpd::LLR_PRE_LO, true>)
                        : reinterpret_cast<const void *>(&qpd::llr_front_kernel<T, qpd::LLR_PRE_LO, false>);
        case qpd::LLR_I32: return reinterpret_cast<const void *>(&qpd::llr_front_kernel<T, qpd::LLR_I32, false>);
        default: return reinterpret_cast<const void *>(&qpd::llr_front_kernel<T, qpd::LLR_U8, false>);
    }
}

// The front kernel on Bc frames of LLRs at `llr`, output `form` (qpd::LlrOut) at
// `out`; timed as the pre-pass, whose place it takes (QPD_KC_PRE).
int llr_front(qpd_decoder *d, qpd::LlrFront C, const void *llr, int32_t type, int64_t Bc, void *out, int form,
              hipStream_t st) {
    const int epl = (int)(16 / llr_size(type));
    C.vec = ((uintptr_t)llr & 15u) == 0;  // N is even, N >= 16 in LLR_PRE: rows, halves and groups keep the base's alignment
    C.out_vec = ((uintptr_t)out & (uintptr_t)(epl - 1)) == 0;
    // LLR_PRE: one thread per output word; else one per 16 bytes of LLRs, four in flight
    const int64_t work = form == qpd::LLR_PRE || form == qpd::LLR_PRE_LO ? (Bc << (d->n - 4)) : (Bc * d->N / epl + 3) / 4;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((work + 255) / 256, 8192));
    const void *kfn = type == QPD_LLR_F32 ? llr_kernel<float>(form, d->llr_coop) : llr_kernel<double>(form, d->llr_coop);
    void *args[] = {&C, &llr, &Bc, &out};
    return timed_launch(d, QPD_KC_PRE, st, [&]() -> int {
        QPD_HIP(hipLaunchKernel(kfn, dim3(grid), dim3(256), args, 0, st));
        QPD_HIP(hipGetLastError());
        return QPD_OK;
    });
}

// qpd_decode_llr's work on stream st (caller: lock held, stream ordered; q <= v).
// Pre-mode: the front kernel writes the root pre-pass rows of a chunk, the decode
// reads them (as mc_decode's fused branch).  Everything else: int32 symbols into
// the staging chunk qpd_decode_u8 widens into, and the int32 launch.
int decode_llr_impl(qpd_decoder *d, const qpd_mc_channel *ch, const void *d_llr, int32_t type, int64_t B, uint8_t *d_out,
                    hipStream_t st) {
    const bool pre = d->engine == QPD_ENGINE_FAST && d->pre;
    d->last_engine = QPD_RAN_GPU;
    d->u8_staged = 0;
    int rc = QPD_OK;
    const int64_t chunk = pre ? reserve_pre_rows(d, B, &rc)
                              : reserve_symbols(d, d->u8_sym, B, d->u8_chunk, "LLR staging hipMalloc: ", &rc);
    if (rc) return rc;
    const qpd::LlrFront C = llr_front_args(d, ch);
    void *buf = pre ? d->pre_rows.p : d->u8_sym.p;
    const size_t row = (size_t)d->N * llr_size(type);
    for (int64_t f0 = 0; f0 < B; f0 += chunk) {
        const int64_t Bc = std::min<int64_t>(chunk, B - f0);
        if ((rc = llr_front(d, C, (const char *)d_llr + f0 * row, type, Bc, buf,
                            pre ? (d->row_lo ? qpd::LLR_PRE_LO : qpd::LLR_PRE) : qpd::LLR_I32, st)))
            return rc;
        uint8_t *out = d_out + f0 * d->out_bits;
        rc = pre ? decode_pre_rows(d, (const uint32_t *)buf, Bc, out, st) : decode_impl(d, (const int32_t *)buf, Bc, out, st);
        if (rc) return rc;
    }
    return QPD_OK;
}

// The host-buffer call's quantizer: B * N LLRs to bytes with the kernel's own
// function.  Returns the error flags (ERR_NAN_LLR: a NaN, stored as symbol 0).
template <class T>
int32_t quantize_llr_host(const qpd_mc_channel *ch, const T *llr, int64_t n, uint8_t *sym) {
    const qpd::LlrQuant Q = qpd::llr_quant_params(ch->edges, ch->n_edges, ch->q);
    double E[qpd::kLlrMaxEdges + 1];
    qpd::llr_guard_edges(ch->edges, ch->n_edges, E);
    int32_t flag = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int s = qpd::quantize_llr((double)llr[i], Q, E, ch->lut);
        if (s < 0) flag |= qpd::ERR_NAN_LLR;
        sym[i] = (uint8_t)(s < 0 ? 0 : s);
    }
    return flag;
}

}  // namespace
