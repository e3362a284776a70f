// qpd_capi.hip -- C-ABI of libqpd.so (include/qpd.h): the extern "C" entry
// points.  What they call, by concern: the handle and the ordering of its work
// (qpd_decoder.hpp), qpd_create's decisions (qpd_config.hpp) and steps
// (qpd_capi_build.hpp), the device-buffer decodes (qpd_capi_decode.hpp), the
// host-buffer ones (qpd_capi_host.hpp), the Monte-Carlo front end
// (qpd_capi_mc.hpp), the LLR front end (qpd_capi_llr.hpp), the transmit side
// (qpd_capi_tx.hpp).  Host code only; this
// unit also compiles the small kernels (root pre-pass, widening copy,
// Monte-Carlo, LLR quantizer, LDS probe); the decode
// kernels are in qpd_generic.hip / qpd_fast.hip and their units, the transmit
// kernels in qpd_tx.hip.
#include <hip/hip_runtime.h>

#include "qpd.h"
#include "qpd_generic.hip"
#include "qpd_fast_plan.hpp"
#include "qpd_fast_pre.hpp"
#include "qpd_mc.hip"
#include "qpd_llr.hip"
#include "qpd_probe.hip"

#include "qpd_decoder.hpp"
#include "qpd_dmetric.hpp"
#include "qpd_capi_build.hpp"
#include "qpd_capi_decode.hpp"
#include "qpd_capi_host.hpp"
#include "qpd_capi_mc.hpp"
#include "qpd_capi_llr.hpp"
#include "qpd_capi_tx.hpp"

namespace {

// The checks of both status entry points: the request, then the decode's own.
int check_status_call(const qpd_decoder *d, int32_t in_type, const qpd_status_args *sa, const char *suffix,
                             int64_t B, const void *in, const void *out, qpd_stat::Req *rq, bool *run) {
    *run = false;
    if (!d) return fail(QPD_E_INVALID, "null decoder");
    std::string err;
    const int rc = qpd_stat::check(d->pub_kind, d->L, d->crc_n, in_type, sa, rq, err);
    if (rc) return fail(rc, err);
    return check_decode_args(d, in_type != QPD_IN_F64, suffix, B, in, out, run);
}

template <class Eng, class In>
int status_host(qpd_decoder *d, Eng *eng, const In *h_in, int32_t in_type, int64_t B, uint8_t *h_out,
                       const qpd_stat::Req &rq) {
    if (host_engine_takes(d, B)) {
        std::lock_guard<std::mutex> lk(d->mu);
        d->last_engine = QPD_RAN_HOST;
        d->u8_staged = 0;
        const int32_t flag = qpd_stat::host_run(eng, h_in, B, d->N, d->out_bits, h_out, rq);
        return flag ? input_error(flag) : QPD_OK;
    }
    // the GPU: metrics and flags through a device buffer of the handle, copied back on
    // its stream before host_roundtrip's synchronization
    return host_roundtrip(d, h_in, B, h_out, [&](const In *in, uint8_t *out, hipStream_t hs) -> int {
        int rc = ensure(d->h_st, d->h_st_bytes, (size_t)B * 9);
        if (rc) return rc;
        qpd_stat::Req dev = rq;
        if (rq.metric) dev.metric = (double *)d->h_st.p;
        if (rq.pass) dev.pass = (uint8_t *)d->h_st.p + (size_t)B * 8;
        {
            StatusScope sc(d, dev, out);
            rc = decode_typed(d, in, in_type, B, out, hs);
        }
        if (rc) return rc;
        if (rq.metric) QPD_HIP(hipMemcpyAsync(rq.metric, dev.metric, (size_t)B * 8, hipMemcpyDeviceToHost, hs));
        if (rq.pass) QPD_HIP(hipMemcpyAsync(rq.pass, dev.pass, (size_t)B, hipMemcpyDeviceToHost, hs));
        return QPD_OK;
    });
}

// The checks of both list entry points: the request (qpd_list.hpp), then the decode's
// own, with the bits optional.
int check_list_call(const qpd_decoder *d, int32_t in_type, const qpd_list_args *la, const char *suffix, int64_t B,
                    const void *in, qpd_list::Req *rq, bool *run) {
    *run = false;
    if (!d) return fail(QPD_E_INVALID, "null decoder");
    std::string err;
    const int rc = qpd_list::check(d->pub_kind, d->L, d->crc_n, in_type, la, rq, err);
    if (rc) return fail(rc, err);
    return check_decode_args(d, in_type != QPD_IN_F64, suffix, B, in, rq->bits, run);
}

// One device-buffer list decode (caller: lock held, stream ordered): into d_out, or
// into a buffer of the handle where the call gave none (a launch finds its first
// frame from where it writes its bits, list_at).
int decode_list_typed(qpd_decoder *d, const void *d_in, int32_t in_type, int64_t B, uint8_t *d_out,
                      const qpd_list::Req &rq, hipStream_t st) {
    if (!d_out) {
        const int rc = ensure(d->ls_out, d->ls_out_bytes, (size_t)B * d->out_bits);
        if (rc) return rc;
        d_out = (uint8_t *)d->ls_out.p;
    }
    ListScope sc(d, rq, d_out);
    return decode_typed(d, d_in, in_type, B, d_out, st);
}

template <class Eng, class In>
int list_host(qpd_decoder *d, Eng *eng, const In *h_in, int32_t in_type, int64_t B, uint8_t *h_out,
              const qpd_list::Req &rq) {
    if (host_engine_takes(d, B)) {
        std::lock_guard<std::mutex> lk(d->mu);
        d->last_engine = QPD_RAN_HOST;
        d->u8_staged = 0;
        const int32_t flag = qpd_list::host_run(eng, h_in, B, d->N, d->K, d->L, d->out_bits, h_out, rq);
        return flag ? input_error(flag) : QPD_OK;
    }
    // the GPU: the list through a device buffer of the handle (metrics, chosen, bits,
    // flags: each aligned for its type), copied back on its stream before
    // host_roundtrip's synchronization
    const size_t n = (size_t)B * d->L, nb = n * d->K;
    return host_roundtrip(d, h_in, B, h_out, [&](const In *in, uint8_t *out, hipStream_t hs) -> int {
        int rc = ensure(d->h_ls, d->h_ls_bytes, n * 8 + (size_t)B * 4 + nb + n);
        if (rc) return rc;
        char *base = (char *)d->h_ls.p;
        qpd_list::Req dev = rq;
        dev.bits = (uint8_t *)(base + n * 8 + (size_t)B * 4);
        if (rq.metric) dev.metric = (double *)base;
        if (rq.chosen) dev.chosen = (int32_t *)(base + n * 8);
        if (rq.pass) dev.pass = dev.bits + nb;
        if ((rc = decode_list_typed(d, in, in_type, B, h_out ? out : nullptr, dev, hs))) return rc;  // (no h_out: no staging for it)
        QPD_HIP(hipMemcpyAsync(rq.bits, dev.bits, nb, hipMemcpyDeviceToHost, hs));
        if (rq.metric) QPD_HIP(hipMemcpyAsync(rq.metric, dev.metric, n * 8, hipMemcpyDeviceToHost, hs));
        if (rq.pass) QPD_HIP(hipMemcpyAsync(rq.pass, dev.pass, n, hipMemcpyDeviceToHost, hs));
        if (rq.chosen) QPD_HIP(hipMemcpyAsync(rq.chosen, dev.chosen, (size_t)B * 4, hipMemcpyDeviceToHost, hs));
        return QPD_OK;
    });
}

// The checks of both search entry points: the request (qpd_search.hpp), then the decode's
// own, with the bits optional.
int check_search_call(const qpd_decoder *d, int32_t in_type, const qpd_search_args *sa, const char *suffix, int64_t B,
                      const void *in, const void *out, qpd_search::Req *rq, bool *run) {
    *run = false;
    if (!d) return fail(QPD_E_INVALID, "null decoder");
    std::string err;
    const int rc = qpd_search::check(d->pub_kind, d->L, d->K, d->ca_A, d->crc_n, in_type, sa, out != nullptr, rq, err);
    if (rc) return fail(rc, err);
    return check_decode_args(d, in_type != QPD_IN_F64, suffix, B, in, d, run);  // (no required output)
}

// One device-buffer search decode (caller: lock held, stream ordered): as decode_list_typed.
int decode_search_typed(qpd_decoder *d, const void *d_in, int32_t in_type, int64_t B, uint8_t *d_out,
                        const qpd_search::Req &rq, hipStream_t st) {
    uint8_t *base = d_out;
    if (!base) {  // a launch finds its first frame from where it would write its bits (search_at)
        const int rc = ensure(d->ls_out, d->ls_out_bytes, (size_t)B * d->out_bits);
        if (rc) return rc;
        base = (uint8_t *)d->ls_out.p;
    }
    SearchScope sc(d, rq, base);
    if (sc.rc) return sc.rc;
    return decode_typed(d, d_in, in_type, B, base, st);
}

template <class Eng, class In>
int search_host(qpd_decoder *d, Eng *eng, const In *h_in, int32_t in_type, int64_t B, uint8_t *h_out,
                const qpd_search::Req &rq) {
    if (host_engine_takes(d, B)) {
        std::lock_guard<std::mutex> lk(d->mu);
        d->last_engine = QPD_RAN_HOST;
        d->u8_staged = 0;
        const int32_t flag = qpd_search::host_run(eng, h_in, B, d->N, d->L, d->out_bits, h_out, rq);
        return flag ? input_error(flag) : QPD_OK;
    }
    // the GPU: the results through a device buffer of the handle (metrics, then the 32-bit
    // outputs: each aligned for its type), copied back on its stream before
    // host_roundtrip's synchronization
    const size_t n = (size_t)B * d->L, nb = (size_t)B;
    return host_roundtrip(d, h_in, B, h_out, [&](const In *in, uint8_t *out, hipStream_t hs) -> int {
        int rc = ensure(d->h_sr, d->h_sr_bytes, n * 8 + nb * 8 + n * 4 + nb * 8);
        if (rc) return rc;
        char *base = (char *)d->h_sr.p;
        qpd_search::Req dev = rq;
        if (rq.cand_metric) dev.cand_metric = (double *)base;
        if (rq.metric) dev.metric = (double *)(base + n * 8);
        if (rq.syndrome) dev.syndrome = (uint32_t *)(base + n * 8 + nb * 8);
        if (rq.hit_mask) dev.hit_mask = (int32_t *)(base + n * 8 + nb * 8 + n * 4);
        if (rq.hit_rank) dev.hit_rank = (int32_t *)(base + n * 8 + nb * 8 + n * 4 + nb * 4);
        if ((rc = decode_search_typed(d, in, in_type, B, h_out ? out : nullptr, dev, hs))) return rc;
        if (rq.cand_metric) QPD_HIP(hipMemcpyAsync(rq.cand_metric, dev.cand_metric, n * 8, hipMemcpyDeviceToHost, hs));
        if (rq.metric) QPD_HIP(hipMemcpyAsync(rq.metric, dev.metric, nb * 8, hipMemcpyDeviceToHost, hs));
        if (rq.syndrome) QPD_HIP(hipMemcpyAsync(rq.syndrome, dev.syndrome, n * 4, hipMemcpyDeviceToHost, hs));
        if (rq.hit_mask) QPD_HIP(hipMemcpyAsync(rq.hit_mask, dev.hit_mask, nb * 4, hipMemcpyDeviceToHost, hs));
        if (rq.hit_rank) QPD_HIP(hipMemcpyAsync(rq.hit_rank, dev.hit_rank, nb * 4, hipMemcpyDeviceToHost, hs));
        return QPD_OK;
    });
}

// The checks of both D-metric entry points (qpd_dmetric.hpp), before any launch.
// *run = false where there is nothing to compute (a refusal, or an empty batch).
int check_dmetric_call(const qpd_decoder *d, int64_t B, const void *in, const void *metric, bool *run) {
    *run = false;
    if (!d) return fail(QPD_E_INVALID, "null decoder");
    std::string err;
    const int rc = qpd_dm::check(d->pub_kind, metric, err);
    if (rc) return fail(rc, err);
    if (B < 0) return fail(QPD_E_INVALID, "negative batch");
    if (B == 0) return QPD_OK;
    if (!in) return fail(QPD_E_INVALID, "null buffer");
    *run = true;
    return QPD_OK;
}

}  // namespace

extern "C" {

int qpd_abi_version(void) { return QPD_ABI_VERSION; }

// Source hash of the tree this library was built from (build.py:
// source_hash); the tagged string is also found in the file's bytes.
#ifndef QPD_BUILD_ID
#define QPD_BUILD_ID "unstamped-build"
#endif
__attribute__((used)) static const char kBuildIdTag[] = "qpd-build-id:" QPD_BUILD_ID;

const char *qpd_build_id(void) { return kBuildIdTag + sizeof("qpd-build-id:") - 1; }

const char *qpd_last_error(void) { return g_err.c_str(); }

int qpd_create(const qpd_config *cfg, qpd_decoder **out) {
    if (!out) return fail(QPD_E_INVALID, "null output handle");
    *out = nullptr;
    int n = 0, fam = 0, dom = 0;
    std::string err;
    int rc = qpd_cfg::validate(cfg, &n, &fam, &dom, err);
    if (rc) return fail(rc, err);
    if (cfg->device >= 0) QPD_HIP(hipSetDevice(cfg->device));
    std::unique_ptr<qpd_decoder> d;  // a failure's ~qpd_decoder waits and frees on that device
    if ((rc = create_decoder(cfg, fam, n, dom, d))) return rc;
    *out = d.release();
    return QPD_OK;
}

void qpd_destroy(qpd_decoder *d) {
    if (!d) return;
    if (d->device >= 0) (void)hipSetDevice(d->device);
    delete d;  // ~qpd_decoder waits for the decoder's last work before any buffer is freed
}

int qpd_get_info(const qpd_decoder *d, qpd_info *info) {
    if (!d || !info) return fail(QPD_E_INVALID, "null argument");
    const bool fast = d->engine == QPD_ENGINE_FAST;
    info->kind = d->pub_kind;
    info->out_bits = d->out_bits;
    info->host_max_frames = !d->hplan ? 0 : d->host_mode == QPD_HOST_GPU ? 0
                            : d->host_mode == QPD_HOST_CPU ? INT64_MAX : d->host_max_frames;
    info->N = d->N;
    info->K = d->K;
    info->L = d->L;
    info->v = d->v;
    info->num_ops = fast ? d->num_mops : (int32_t)d->ops_host.size();
    info->frames_per_wave = fast ? d->plan.fpw * d->sets : d->plan.fpw;
    info->lanes_per_frame = d->plan.gs;
    info->max_waves = d->max_waves;
    info->scratch_bytes_per_wave = d->scratch_bytes_per_wave;
    info->engine = d->engine;
    info->lds_bytes_per_wave = d->lds_bytes;
    info->lds_from_depth = fast ? d->fplan.lds_from : -1;
    info->prefix_ops = fast ? d->prefix_ops() : 0;
    info->last_engine = d->last_engine;
    // f / g ops of a node at depth d look up N >> (d + 1) symbols each; a leaf
    // pair's two decisions one each (SCLLUTDecoder.cpp:83-89, :157-164)
    int64_t lk = 0;
    for (const Op &o : d->ops_host)
        if (o.type == qpd::OP_F || o.type == qpd::OP_G) lk += d->N >> (o.d + 1);
        else if (o.type == qpd::OP_LEAF_L || o.type == qpd::OP_LEAF_R) lk += 1;
    info->lookups_per_path = lk;
    info->fast_variant = fast ? (d->pw1 ? 1 : 0) | (d->r1l ? 2 : 0) : 0;
    info->u8_staged = d->u8_staged;
    return QPD_OK;
}

int qpd_decode(qpd_decoder *d, const int32_t *d_symbols, int64_t B, uint8_t *d_out, void *stream) {
    bool run;
    const int rc = check_decode_args(d, true, "", B, d_symbols, d_out, &run);
    if (!run) return rc;
    hipStream_t st = (hipStream_t)stream;
    return ordered(d, st, [&]() { return decode_impl(d, d_symbols, B, d_out, st); });
}

int qpd_decode_u8(qpd_decoder *d, const uint8_t *d_symbols, int64_t B, uint8_t *d_out, void *stream) {
    bool run;
    const int rc = check_decode_args(d, true, "", B, d_symbols, d_out, &run);
    if (!run) return rc;
    hipStream_t st = (hipStream_t)stream;
    return ordered(d, st, [&]() { return decode_u8_impl(d, d_symbols, B, d_out, st); });
}

int qpd_decode_f64(qpd_decoder *d, const double *d_llr, int64_t B, uint8_t *d_out, void *stream) {
    bool run;
    const int rc = check_decode_args(d, false, "", B, d_llr, d_out, &run);
    if (!run) return rc;
    hipStream_t st = (hipStream_t)stream;
    return ordered(d, st, [&]() { return decode_f64_impl(d, d_llr, B, d_out, st); });
}

int qpd_decode_status(qpd_decoder *d, const void *d_in, int32_t in_type, int64_t B, uint8_t *d_out,
                      const qpd_status_args *sa, void *stream) {
    bool run;
    qpd_stat::Req rq;
    const int rc = check_status_call(d, in_type, sa, "", B, d_in, d_out, &rq, &run);
    if (!run) return rc;
    hipStream_t st = (hipStream_t)stream;
    return ordered(d, st, [&]() {
        StatusScope sc(d, rq, d_out);
        return decode_typed(d, d_in, in_type, B, d_out, st);
    });
}

int qpd_decode_status_host(qpd_decoder *d, const void *h_in, int32_t in_type, int64_t B, uint8_t *h_out,
                           const qpd_status_args *sa) {
    bool run;
    qpd_stat::Req rq;
    const int rc = check_status_call(d, in_type, sa, "_host", B, h_in, h_out, &rq, &run);
    if (!run) return rc;
    switch (in_type) {
        case QPD_IN_I32: return status_host(d, d->heng_lut.get(), (const int32_t *)h_in, in_type, B, h_out, rq);
        case QPD_IN_U8: return status_host(d, d->heng_lut.get(), (const uint8_t *)h_in, in_type, B, h_out, rq);
        default: return status_host(d, d->heng_f64.get(), (const double *)h_in, in_type, B, h_out, rq);
    }
}

int qpd_decode_list(qpd_decoder *d, const void *d_in, int32_t in_type, int64_t B, uint8_t *d_out,
                    const qpd_list_args *la, void *stream) {
    bool run;
    qpd_list::Req rq;
    const int rc = check_list_call(d, in_type, la, "", B, d_in, &rq, &run);
    if (!run) return rc;
    hipStream_t st = (hipStream_t)stream;
    return ordered(d, st, [&]() { return decode_list_typed(d, d_in, in_type, B, d_out, rq, st); });
}

int qpd_decode_list_host(qpd_decoder *d, const void *h_in, int32_t in_type, int64_t B, uint8_t *h_out,
                         const qpd_list_args *la) {
    bool run;
    qpd_list::Req rq;
    const int rc = check_list_call(d, in_type, la, "_host", B, h_in, &rq, &run);
    if (!run) return rc;
    switch (in_type) {
        case QPD_IN_I32: return list_host(d, d->heng_lut.get(), (const int32_t *)h_in, in_type, B, h_out, rq);
        case QPD_IN_U8: return list_host(d, d->heng_lut.get(), (const uint8_t *)h_in, in_type, B, h_out, rq);
        default: return list_host(d, d->heng_f64.get(), (const double *)h_in, in_type, B, h_out, rq);
    }
}

int qpd_decode_search(qpd_decoder *d, const void *d_in, int32_t in_type, int64_t B, uint8_t *d_out,
                      const qpd_search_args *sa, void *stream) {
    bool run;
    qpd_search::Req rq;
    const int rc = check_search_call(d, in_type, sa, "", B, d_in, d_out, &rq, &run);
    if (!run) return rc;
    hipStream_t st = (hipStream_t)stream;
    return ordered(d, st, [&]() { return decode_search_typed(d, d_in, in_type, B, d_out, rq, st); });
}

int qpd_decode_search_host(qpd_decoder *d, const void *h_in, int32_t in_type, int64_t B, uint8_t *h_out,
                           const qpd_search_args *sa) {
    bool run;
    qpd_search::Req rq;
    const int rc = check_search_call(d, in_type, sa, "_host", B, h_in, h_out, &rq, &run);
    if (!run) return rc;
    switch (in_type) {
        case QPD_IN_I32: return search_host(d, d->heng_lut.get(), (const int32_t *)h_in, in_type, B, h_out, rq);
        case QPD_IN_U8: return search_host(d, d->heng_lut.get(), (const uint8_t *)h_in, in_type, B, h_out, rq);
        default: return search_host(d, d->heng_f64.get(), (const double *)h_in, in_type, B, h_out, rq);
    }
}

int qpd_check_input_error(qpd_decoder *d) {
    if (!d) return fail(QPD_E_INVALID, "null decoder");
    hipStream_t hs = d->hs;
    return ordered(d, hs, [&]() -> int {
        int32_t flag = 0;
        QPD_HIP(hipMemcpyAsync(&flag, d->err.p, sizeof(flag), hipMemcpyDeviceToHost, hs));
        QPD_HIP(hipStreamSynchronize(hs));
        return take_input_error(d, flag);
    });
}

int qpd_decode_host(qpd_decoder *d, const int32_t *h_symbols, int64_t B, uint8_t *h_out) {
    bool run;
    const int rc = check_decode_args(d, true, "_host", B, h_symbols, h_out, &run);
    if (!run) return rc;
    return host_decode(d, d->heng_lut.get(), h_symbols, B, h_out,
                       [&](const int32_t *in, uint8_t *out, hipStream_t st) { return decode_impl(d, in, B, out, st); });
}

int qpd_decode_u8_host(qpd_decoder *d, const uint8_t *h_symbols, int64_t B, uint8_t *h_out) {
    bool run;
    const int rc = check_decode_args(d, true, "_host", B, h_symbols, h_out, &run);
    if (!run) return rc;
    return host_decode(d, d->heng_lut.get(), h_symbols, B, h_out,
                       [&](const uint8_t *in, uint8_t *out, hipStream_t st) { return decode_u8_impl(d, in, B, out, st); });
}

int qpd_decode_f64_host(qpd_decoder *d, const double *h_llr, int64_t B, uint8_t *h_out) {
    bool run;
    const int rc = check_decode_args(d, false, "_host", B, h_llr, h_out, &run);
    if (!run) return rc;
    return host_decode(d, d->heng_f64.get(), h_llr, B, h_out,
                       [&](const double *in, uint8_t *out, hipStream_t st) { return decode_f64_impl(d, in, B, out, st); });
}

int qpd_dmetric(qpd_decoder *d, const double *d_llr, int64_t B, double *d_metric, uint8_t *d_out, void *stream) {
    bool run;
    const int rc = check_dmetric_call(d, B, d_llr, d_metric, &run);
    if (!run) return rc;
    hipStream_t st = (hipStream_t)stream;
    return ordered(d, st, [&]() { return decode_f64_impl(d, d_llr, B, d_out, st, d_metric); });
}

int qpd_dmetric_host(qpd_decoder *d, const double *h_llr, int64_t B, double *h_metric, uint8_t *h_out) {
    bool run;
    const int rc = check_dmetric_call(d, B, h_llr, h_metric, &run);
    if (!run) return rc;
    if (host_engine_takes(d, B)) {
        std::lock_guard<std::mutex> lk(d->mu);
        d->last_engine = QPD_RAN_HOST;
        d->u8_staged = 0;
        const int32_t flag = qpd_dm::host_run(d->heng_f64.get(), h_llr, B, d->N, d->out_bits, h_metric, h_out);
        return flag ? input_error(flag) : QPD_OK;
    }
    // the GPU: the metrics through a device buffer of the handle, copied back on its
    // stream before host_roundtrip's synchronization
    return host_roundtrip(d, h_llr, B, h_out, [&](const double *in, uint8_t *out, hipStream_t hs) -> int {
        int r = ensure(d->h_st, d->h_st_bytes, (size_t)B * sizeof(double));
        if (r) return r;
        if ((r = decode_f64_impl(d, in, B, h_out ? out : nullptr, hs, (double *)d->h_st.p))) return r;
        QPD_HIP(hipMemcpyAsync(h_metric, d->h_st.p, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, hs));
        return QPD_OK;
    });
}

int qpd_quantize_llr(qpd_decoder *d, const qpd_mc_channel *ch, const void *d_llr, int32_t llr_type, int64_t B,
                     uint8_t *d_symbols, void *stream) {
    bool run;
    const int rc = check_llr_args(d, ch, d_llr, llr_type, B, d_symbols, 256, "qpd_quantize_llr: q must be at most 256", &run);
    if (!run) return rc;
    hipStream_t st = (hipStream_t)stream;
    return ordered(d, st, [&]() { return llr_front(d, llr_front_args(d, ch), d_llr, llr_type, B, d_symbols, qpd::LLR_U8, st); });
}

int qpd_decode_llr(qpd_decoder *d, const qpd_mc_channel *ch, const void *d_llr, int32_t llr_type, int64_t B,
                   uint8_t *d_out, void *stream) {
    bool run;
    const int rc = check_llr_args(d, ch, d_llr, llr_type, B, d_out, -1, "qpd_decode_llr: q must be at most the decoder's v", &run);
    if (!run) return rc;
    hipStream_t st = (hipStream_t)stream;
    return ordered(d, st, [&]() { return decode_llr_impl(d, ch, d_llr, llr_type, B, d_out, st); });
}

int qpd_decode_llr_host(qpd_decoder *d, const qpd_mc_channel *ch, const void *h_llr, int32_t llr_type, int64_t B,
                        uint8_t *h_out) {
    bool run;
    int rc = check_llr_args(d, ch, h_llr, llr_type, B, h_out, -1, "qpd_decode_llr_host: q must be at most the decoder's v", &run);
    if (!run) return rc;
    std::vector<uint8_t> sym((size_t)B * d->N);
    const int32_t flag = llr_type == QPD_LLR_F32 ? quantize_llr_host(ch, (const float *)h_llr, B * d->N, sym.data())
                                                 : quantize_llr_host(ch, (const double *)h_llr, B * d->N, sym.data());
    rc = host_decode(d, d->heng_lut.get(), sym.data(), B, h_out, [&](const uint8_t *in, uint8_t *out, hipStream_t st) {
        const int r = decode_u8_impl(d, in, B, out, st);
        d->u8_staged = 0;  // the staging is this call's own business: qpd_info.u8_staged is about uint8 input
        return r;
    });
    return rc ? rc : flag ? input_error(flag) : QPD_OK;
}

int qpd_set_host_engine(qpd_decoder *d, int32_t mode) {
    if (!d) return fail(QPD_E_INVALID, "null decoder");
    if (mode < QPD_HOST_AUTO || mode > QPD_HOST_CPU) return fail(QPD_E_INVALID, "mode must be QPD_HOST_AUTO, _GPU or _CPU");
    if (mode == QPD_HOST_CPU && !d->hplan)
        return fail(QPD_E_UNSUPPORTED, "the host engine does not decode the re-quantized float kinds");
    std::lock_guard<std::mutex> lk(d->mu);
    d->host_mode = mode;
    return QPD_OK;
}

int qpd_mc_frames(qpd_decoder *d, const qpd_mc_channel *ch, uint64_t seed, int64_t frame0, int64_t B, uint8_t *d_msg,
                  int32_t *d_symbols, void *stream) {
    bool run;
    const int rc = check_mc_args(d, ch, false, frame0, B, d_msg, d_symbols, &run);
    if (!run) return rc;
    hipStream_t st = (hipStream_t)stream;
    return ordered(d, st, [&]() { return mc_launch(d, ch, seed, frame0, B, d_msg, d_symbols, qpd::MC_SYM, st); });
}

int qpd_mc_decode(qpd_decoder *d, const qpd_mc_channel *ch, uint64_t seed, int64_t frame0, int64_t B, uint8_t *d_msg,
                  uint8_t *d_out, int64_t *d_counts, void *stream) {
    bool run;
    const int rc = check_mc_args(d, ch, true, frame0, B, d_msg, d_out, &run);
    if (!run) return rc;
    hipStream_t st = (hipStream_t)stream;
    return ordered(d, st, [&]() { return mc_decode(d, ch, seed, frame0, B, d_msg, d_out, d_counts, st); });
}

int qpd_mc_llr(qpd_decoder *d, const qpd_mc_channel *ch, const double *rec, uint64_t seed, int64_t frame0, int64_t B,
               uint8_t *d_msg, double *d_llr, void *stream) {
    bool run;
    const int rc = check_mc_llr_args(d, ch, rec, false, frame0, B, d_msg, d_llr, &run);
    if (!run) return rc;
    hipStream_t st = (hipStream_t)stream;
    return ordered(d, st, [&]() {
        return mc_launch(d, ch, seed, frame0, B, d_msg, d_llr, rec ? qpd::MC_LLR_REC : qpd::MC_LLR, st, rec);
    });
}

int qpd_mc_decode_f64(qpd_decoder *d, const qpd_mc_channel *ch, const double *rec, uint64_t seed, int64_t frame0,
                      int64_t B, uint8_t *d_msg, uint8_t *d_out, int64_t *d_counts, void *stream) {
    bool run;
    const int rc = check_mc_llr_args(d, ch, rec, true, frame0, B, d_msg, d_out, &run);
    if (!run) return rc;
    hipStream_t st = (hipStream_t)stream;
    return ordered(d, st, [&]() { return mc_decode_f64(d, ch, rec, seed, frame0, B, d_msg, d_out, d_counts, st); });
}

int qpd_encode(qpd_decoder *d, const uint8_t *d_msg, int64_t B, const qpd_tx_args *tx, uint8_t *d_info, uint8_t *d_codeword,
               void *stream) {
    if (!d) return fail(QPD_E_INVALID, "null decoder");
    bool run;
    uint32_t mask;
    std::string err;
    const int rc = qpd_tx::check_encode(d->pub_kind, d->K, d->ca_A, d->crc_n, tx, B, d_msg, d_info, d_codeword, &mask, &run, err);
    if (rc) return fail(rc, "qpd_encode: " + err);
    if (!run) return QPD_OK;
    hipStream_t st = (hipStream_t)stream;
    return ordered(d, st, [&]() { return tx_encode_launch(d, d_msg, B, mask, d_info, d_codeword, st); });
}

int qpd_encode_host(qpd_decoder *d, const uint8_t *h_msg, int64_t B, const qpd_tx_args *tx, uint8_t *h_info,
                    uint8_t *h_codeword) {
    if (!d) return fail(QPD_E_INVALID, "null decoder");
    bool run;
    uint32_t mask;
    std::string err;
    int rc = qpd_tx::check_encode(d->pub_kind, d->K, d->ca_A, d->crc_n, tx, B, h_msg, h_info, h_codeword, &mask, &run, err);
    if (rc) return fail(rc, "qpd_encode_host: " + err);
    if (!run) return QPD_OK;
    std::lock_guard<std::mutex> lk(d->mu);
    if ((rc = tx_host_code(d))) return rc;
    const int32_t flag = qpd_tx::encode_host(*d->tx_code, h_msg, B, mask, h_info, h_codeword);
    return flag ? input_error(flag) : QPD_OK;
}

int qpd_tx_frames(qpd_decoder *d, const qpd_mc_channel *ch, const double *rec, uint64_t seed, int64_t frame0, int64_t B,
                  const uint8_t *d_msg, const qpd_tx_args *tx, int32_t out_type, void *d_frames, void *stream) {
    if (!d) return fail(QPD_E_INVALID, "null decoder");
    bool run;
    uint32_t mask;
    std::string err;
    int rc = qpd_tx::check_frames(d->pub_kind, d->K, d->ca_A, d->crc_n, tx, frame0, B, d_msg, out_type, ch != nullptr,
                                  ch ? ch->q : 0, rec != nullptr, d_frames, &mask, &run, err);
    if (rc) return fail(rc, "qpd_tx_frames: " + err);
    if (!run) return QPD_OK;
    if ((rc = out_type == QPD_TX_LLR_F64 ? check_llr_channel(ch, rec) : check_channel(ch))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int no_signal = tx && tx->no_signal;
    return ordered(d, st, [&]() {
        return tx_frames_launch(d, ch, rec, seed, frame0, B, d_msg, mask, no_signal, out_type, d_frames, st);
    });
}

int qpd_probe_lds(int32_t device, int32_t op, double *gbps) {
    if (!gbps || op < 0 || op > 2) return fail(QPD_E_INVALID, "bad probe op / null output");
    if (device >= 0) QPD_HIP(hipSetDevice(device));
    QPD_HIP(qpd::probe_lds_run(op, gbps));
    return QPD_OK;
}

int qpd_profile(qpd_decoder *d, int32_t enable) {
    if (!d) return fail(QPD_E_INVALID, "null decoder");
    std::lock_guard<std::mutex> lk(d->mu);
    d->prof = enable != 0;
    return QPD_OK;
}

int qpd_kernel_times(qpd_decoder *d, double *ms, int64_t *launches) {
    if (!d || !ms || !launches) return fail(QPD_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(d->mu);
    int rc = set_device(d);
    if (rc) return rc;
    for (int k = 0; k < QPD_KC_COUNT; ++k) {
        ms[k] = 0.0;
        launches[k] = (int64_t)d->prof_ev[k].size();
        for (auto &e : d->prof_ev[k]) {
            float t = 0.f;
            QPD_HIP(hipEventSynchronize(e.second));
            QPD_HIP(hipEventElapsedTime(&t, e.first, e.second));
            ms[k] += t;
            QPD_HIP(hipEventDestroy(e.first));
            QPD_HIP(hipEventDestroy(e.second));
        }
        d->prof_ev[k].clear();
    }
    return QPD_OK;
}

#ifdef QPD_STAMPS
// Diagnostic builds only (not declared in qpd.h): read and clear the per-class
// cycle / count accumulators of lut_fast_kernel.
int qpd_debug_stamps(unsigned long long *out64) {
    QPD_HIP(hipDeviceSynchronize());
    unsigned long long *acc = stamp_buffer();
    if (!acc) return fail(QPD_E_DEVICE, "stamp buffer");
    QPD_HIP(hipMemcpy(out64, acc, 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    QPD_HIP(hipMemset(acc, 0, 64 * sizeof(unsigned long long)));
    return QPD_OK;
}
#endif
}  // extern "C"
