// qpd_capi_host.hpp -- the host-buffer entry points' two ways: small batches on
// the host engine (qpd_host.hpp), larger ones through pinned staging and the
// device decode; the device error word as a message.  Host code.
#pragma once
#include <cstring>

#include "qpd_decoder.hpp"

namespace {

int input_error(int32_t flag) {
    std::string msg;
    if (flag & qpd::ERR_SYMBOL) msg += "channel symbol outside [0, v) in decoder input; ";
    if (flag & qpd::ERR_LLOYD) msg += "Lloyd bisect index outside the reconstruction list (reference UB); ";
    if (flag & qpd::ERR_NAN_PM) msg += "NaN path metric reached the list sort (reference UB); ";
    if (flag & qpd::ERR_NAN_LLR) msg += "NaN LLR in decoder input (no channel symbol in the reference driver); ";
    if (flag & qpd::ERR_MSG_BIT) msg += "message byte other than 0 or 1 in encoder input (read as its low bit); ";
    msg.resize(msg.size() - 2);
    return fail(QPD_E_INPUT, msg);
}

// `flag`: the device error word as just read on the decoder's own stream hs.
// When set, it is cleared there and reported (caller: ordered on hs, so hs has
// waited for the decoder's last launch on any stream, and later calls on other
// streams wait for the clear).
int take_input_error(qpd_decoder *d, int32_t flag) {
    if (!flag) return QPD_OK;
    QPD_HIP(hipMemsetAsync(d->err.p, 0, sizeof(int32_t), d->hs));
    QPD_HIP(hipStreamSynchronize(d->hs));
    return input_error(flag);
}

int ensure(DeviceBuf &b, size_t &have, size_t need) {
    if (have >= need) return QPD_OK;
    if (b.p) {
        QPD_HIP(hipFree(b.p));
        b.p = nullptr;
    }
    QPD_HIP(hipMalloc(&b.p, need));
    have = need;
    return QPD_OK;
}

// Whether a host-buffer call of B frames runs on the host engine.
bool host_engine_takes(const qpd_decoder *d, int64_t B) {
    if (!d->hplan || d->host_mode == QPD_HOST_GPU) return false;
    return d->host_mode == QPD_HOST_CPU || B <= d->host_max_frames;
}

// B frames on the host engine, one after another, under the handle's lock.
// The GPU work of the decoder is not touched (the engine has its own state),
// so no stream ordering is needed.
template <class Eng, class In>
int host_engine_run(qpd_decoder *d, Eng *eng, const In *h_in, int64_t B, uint8_t *h_out) {
    std::lock_guard<std::mutex> lk(d->mu);
    d->last_engine = QPD_RAN_HOST;
    d->u8_staged = 0;
    int32_t flag = 0;
    for (int64_t b = 0; b < B; ++b) flag |= eng->decode(h_in + b * d->N, h_out + b * d->out_bits);
    return flag ? input_error(flag) : QPD_OK;
}

// One synchronous host-buffer decode: input staged through pinned memory,
// H2D copy, decode and D2H copies of the bits and the error word queued on
// the handle's own stream, one stream synchronization.  (What a per-frame
// decode(symbols) call of the reference drivers costs here: tools/latency.py.)
// h_out == NULL (qpd_dmetric_host without bits): no bits are copied back.
template <class In, class Dec>
int host_roundtrip(qpd_decoder *d, const In *h_in, int64_t B, uint8_t *h_out, Dec dec) {
    const size_t in_b = (size_t)B * d->N * sizeof(In), out_b = h_out ? (size_t)B * d->out_bits : 0;
    const size_t out_at = (in_b + 15) & ~(size_t)15, err_at = out_at + ((out_b + 15) & ~(size_t)15);
    hipStream_t hs = d->hs;
    return ordered(d, hs, [&]() -> int {
        // the staging buffers may still be read by the previous call's work
        // only if that ran on hs, which the synchronization below has drained
        int rc = ensure(d->h_in, d->h_in_bytes, in_b);
        if (rc) return rc;
        if ((rc = ensure(d->h_out, d->h_out_bytes, std::max<size_t>(1, out_b)))) return rc;
        if (d->pin_bytes < err_at + 16) {
            if (d->pin) QPD_HIP(hipHostFree(d->pin));
            d->pin = nullptr;
            d->pin_bytes = 0;
            QPD_HIP(hipHostMalloc(&d->pin, err_at + 16, hipHostMallocDefault));
            d->pin_bytes = err_at + 16;
        }
        char *pin = (char *)d->pin;
        std::memcpy(pin, h_in, in_b);
        QPD_HIP(hipMemcpyAsync(d->h_in.p, pin, in_b, hipMemcpyHostToDevice, hs));
        if ((rc = dec((const In *)d->h_in.p, (uint8_t *)d->h_out.p, hs))) return rc;
        if (out_b) QPD_HIP(hipMemcpyAsync(pin + out_at, d->h_out.p, out_b, hipMemcpyDeviceToHost, hs));
        QPD_HIP(hipMemcpyAsync(pin + err_at, d->err.p, sizeof(int32_t), hipMemcpyDeviceToHost, hs));
        QPD_HIP(hipStreamSynchronize(hs));
        if (out_b) std::memcpy(h_out, pin + out_at, out_b);
        int32_t flag = 0;
        std::memcpy(&flag, pin + err_at, sizeof(flag));
        return take_input_error(d, flag);
    });
}

// A host-buffer decode of B > 0 frames: on the host engine `eng` where it
// takes the batch, else through the device decode `dec`.
template <class Eng, class In, class Dec>
int host_decode(qpd_decoder *d, Eng *eng, const In *h_in, int64_t B, uint8_t *h_out, Dec dec) {
    if (host_engine_takes(d, B)) return host_engine_run(d, eng, h_in, B, h_out);
    return host_roundtrip(d, h_in, B, h_out, dec);
}

}  // namespace
