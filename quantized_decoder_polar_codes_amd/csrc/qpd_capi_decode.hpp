// qpd_capi_decode.hpp -- the launches of one device-buffer decode on a stream
// (caller: lock held, stream ordered -- qpd_decoder.hpp: ordered): int32,
// uint8 and f64 input, the generic engine, the fast engine with its root
// pre-pass and frozen-prefix stages.  Host code.
#pragma once
#include "qpd_capi_build.hpp"
#include "qpd_decoder.hpp"
#include "qpd_fast_pre.hpp"

namespace {

// The stage whose records an import op reads, from the planner's encoding in op.node
// (plan_prefix in qpd_plan.hpp; tests/test_plan.py pins it): 1 = stage 1, 2 = stage 2,
// 3 = stage 1b -- not the stages' order in qpd_decoder::pfx.
int import_stage(const qpd::MOp &m) { return m.node == 3 ? 1 : m.node == 2 ? 2 : 0; }

// Point the import ops of a prefix-split schedule at the stage buffers, on the launch
// stream, when a buffer moved.
int patch_imports(qpd_decoder *d, hipStream_t st) {
    bool moved = false;
    for (const auto &sg : d->pfx) moved = moved || sg.patched != sg.buf.p;
    if (!moved) return QPD_OK;
    auto patch = [&](std::vector<qpd::MOp> &v) {
        for (qpd::MOp &m : v)
            if (m.type == qpd::OP_IMPORT && (m.flags & qpd::MF_XBUF)) {
                const uint64_t a = (uint64_t)(uintptr_t)d->pfx[import_stage(m)].buf.p;
                m.u_row = (int32_t)(uint32_t)a;
                m.r_row = (int32_t)(uint32_t)(a >> 32);
            }
    };
    patch(d->pfx_ops_host);
    patch(d->main_ops_host);
    QPD_HIP(hipMemcpyAsync(d->pfx_mops.p, d->pfx_ops_host.data(), d->pfx_ops_host.size() * sizeof(qpd::MOp),
                           hipMemcpyHostToDevice, st));
    QPD_HIP(hipMemcpyAsync(d->mops.p, d->main_ops_host.data(), d->main_ops_host.size() * sizeof(qpd::MOp),
                           hipMemcpyHostToDevice, st));
    for (auto &sg : d->pfx) sg.patched = sg.buf.p;
    return QPD_OK;
}

// A stage's record buffer for Bc frames (rounded up to whole 64-frame groups), grown on demand.
// (No smaller size on an allocation failure, unlike the chunk buffers: ADVICE.md.)
int ensure_records(DeviceBuf &b, size_t &cap, int64_t Bc, int rec, int paths) {
    const size_t need = (size_t)((Bc + 63) / 64 * 64) * (size_t)rec * paths * sizeof(uint32_t);
    if (cap >= need) return QPD_OK;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    cap = 0;
    const hipError_t e = hipMalloc(&b.p, need);
    if (e != hipSuccess) return fail(QPD_E_DEVICE, std::string("prefix records hipMalloc: ") + hipGetErrorString(e));
    cap = need;
    return QPD_OK;
}

// The status fields of a launch's plan during qpd_decode_status (nothing asked,
// every other call: zeros): the call's outputs from the launch's first frame on,
// which follows from where in the call's d_out the launch writes.
template <class Plan>
void status_at(const qpd_decoder *d, const uint8_t *out, Plan &P) {
    const qpd_stat::Req &rq = d->st_req;
    const int64_t f0 = rq.any() && out ? (out - d->st_out0) / d->out_bits : 0;
    P.crc_mask = rq.mask;
    P.st_metric = rq.metric ? rq.metric + f0 : nullptr;
    P.st_pass = rq.pass ? rq.pass + f0 : nullptr;
}

// Likewise the list fields during qpd_decode_list (mask: the list call's).
template <class Plan>
void list_at(const qpd_decoder *d, const uint8_t *out, Plan &P) {
    const qpd_list::Req &rq = d->ls_req;
    if (!rq.any()) {
        P.ls_bits = nullptr;
        P.ls_metric = nullptr;
        P.ls_pass = nullptr;
        P.ls_chosen = nullptr;
        return;
    }
    const int64_t f0 = (out - d->st_out0) / d->out_bits;
    P.crc_mask = rq.mask;
    P.ls_bits = rq.bits + f0 * d->L * d->K;
    P.ls_metric = rq.metric ? rq.metric + f0 * d->L : nullptr;
    P.ls_pass = rq.pass ? rq.pass + f0 * d->L : nullptr;
    P.ls_chosen = rq.chosen ? rq.chosen + f0 : nullptr;
}

// Likewise the search fields during qpd_decode_search, over the list fields it shares (cand_metric,
// hit_rank) and the status call's metric.  FS: FastStatus (its sr_* fields) or the generic
// kernels' DevSearch.
template <class Plan>
void search_shared_at(const qpd_decoder *d, int64_t f0, Plan &P) {
    const qpd_search::Req &rq = d->sr_req;
    P.crc_mask = 0;
    P.ls_bits = nullptr;
    P.ls_pass = nullptr;
    P.ls_metric = rq.cand_metric ? rq.cand_metric + f0 * d->L : nullptr;
    P.ls_chosen = rq.hit_rank ? rq.hit_rank + f0 : nullptr;
    P.st_metric = rq.metric ? rq.metric + f0 : nullptr;
    P.st_pass = nullptr;
}
void search_at(const qpd_decoder *d, const uint8_t *out, qpd::FastStatus &so) {
    const qpd_search::Req &rq = d->sr_req;
    const int64_t f0 = (out - d->st_out0) / d->out_bits;
    search_shared_at(d, f0, so);
    so.sr_set = (const uint32_t *)d->sr_set.p;
    so.sr_n = (int32_t)rq.words.size();
    so.sr_syndrome = rq.syndrome ? rq.syndrome + f0 * d->L : nullptr;
    so.sr_hit = rq.hit_mask ? rq.hit_mask + f0 : nullptr;
}
void search_at(const qpd_decoder *d, const uint8_t *out, qpd::DevPlan &P, qpd::DevSearch &sr) {
    const qpd_search::Req &rq = d->sr_req;
    const int64_t f0 = (out - d->st_out0) / d->out_bits;
    search_shared_at(d, f0, P);
    sr.set = (const uint32_t *)d->sr_set.p;
    sr.n = (int32_t)rq.words.size();
    sr.syndrome = rq.syndrome ? rq.syndrome + f0 * d->L : nullptr;
    sr.hit = rq.hit_mask ? rq.hit_mask + f0 : nullptr;
}

// dmetric (qpd_dmetric, a float FastSC decoder): the launch runs the kernel's DM twin, which writes
// the frames' blind-detection metrics there and takes a NULL out; the plain kernels do not read it.
template <class In>
int launch_generic(qpd_decoder *d, const In *in, int64_t B, uint8_t *out, int grid, hipStream_t st,
                   double *dmetric = nullptr) {
    const void *kfn = dmetric            ? qpd::dmetric_kernel()
                      : d->ls_req.any() || d->sr_req.any() ? qpd::generic_list_kernel(d->kind, d->dom, d->L > qpd::kMaxL)
                                        : generic_kernel(d->kind, d->dom, d->L > qpd::kMaxL);
    if (!kfn) return fail(QPD_E_INVALID, "bad kind");
    qpd::DevPlan P = d->plan;
    P.task_base = d->task_base;
    status_at(d, out, P);
    list_at(d, out, P);
    qpd::DevSearch sr{};
    if (d->sr_req.any()) search_at(d, out, P, sr);
    const In *in_arg = in;
    void *args[] = {&P, &in_arg, &B, &out, &dmetric, &sr};
    const int rc = timed_launch(d, QPD_KC_DECODE, st, [&]() -> int {
        QPD_HIP(hipLaunchKernel(kfn, dim3(grid), dim3(64), args, 0, st));
        QPD_HIP(hipGetLastError());
        return QPD_OK;
    });
    if (!rc) d->task_base += (uint32_t)((B + d->plan.fpw - 1) / d->plan.fpw);  // takes of this launch (wave_take)
    return rc;
}

// One fast-engine decode launch over Bc frames whose rows start at `in`
// (channel symbols, in_shift = n; or pre-pass rows, in_shift = n - 2).
int fast_launch(qpd_decoder *d, qpd::FastPlan fp, const int32_t *in, int64_t Bc, uint8_t *out, hipStream_t st,
                bool prefix = false) {
    const int sets = prefix ? d->pfx_sets : d->sets;
    const int64_t tw = (int64_t)fp.fpw * sets;  // frames per wave task
    // a status call's decode launch runs the plan's ST twin (the plain kernels do not read the status fields)
    // ... and a list call's the LIST twin
    // ... and so does a search call's, with the search fields set
    const bool search = !prefix && d->sr_req.any();
    const bool status = !prefix && d->st_req.any(), list = !prefix && (d->ls_req.any() || search);
    const void *kfn = prefix ? prefix_kernel(d->kind, sets, d->pw1)
                             : fast_kernel(d->kind, d->sets, d->l8, d->r1l, d->pw1, d->w16, list ? 2 : status ? 1 : 0);
    if (!kfn) return fail(QPD_E_INVALID, "bad kind");
    qpd::FastStatus so{};
    if (status) status_at(d, out, so);
    if (list) list_at(d, out, so);
    if (search) search_at(d, out, so);
    const int64_t fgroups = (Bc + tw - 1) / tw;
    int fgrid = (int)std::min<int64_t>(fgroups, d->max_waves);
    if (!QPD_DYN) {
        // even out the rounds of the grid-stride loop (no partial last round)
        const int64_t rounds = (fgroups + fgrid - 1) / fgrid;
        fgrid = (int)((fgroups + rounds - 1) / rounds);
    }
    const qpd::MOp *ops_arg = fp.ops;
    fp.task_base = d->task_base;
    void *args[] = {&fp, &in, &Bc, &out, &ops_arg, &so};
    // the prefix stages run pfx_sets frame sets per wave in the same per-set layout
    const size_t lds = (size_t)((d->lds_bytes - d->lds_tab_bytes) / d->sets * sets + d->lds_tab_bytes);
    const int rc = timed_launch(d, prefix ? QPD_KC_PFX : QPD_KC_DECODE, st, [&]() -> int {
        QPD_HIP(hipLaunchKernel(kfn, dim3(fgrid), dim3(64), args, lds, st));
        QPD_HIP(hipGetLastError());
        return QPD_OK;
    });
    if (!rc) d->task_base += (uint32_t)fgroups;  // takes of this launch (wave_take)
    return rc;
}

// FastPlan::pfx_geo of a prefix stage with 2^ps paths per frame: 64 >> ps frames of 2^ps paths per 64 words.
constexpr int prefix_geo(int ps) { return (6 - ps) | (ps << 8); }
static_assert(prefix_geo(0) == 6 && prefix_geo(1) == (5 | (1 << 8)) && prefix_geo(2) == (4 | (2 << 8)), "stages 1, 1b, 2");

// The decode of Bc frames from their root pre-pass rows (pre-mode decoders).
int decode_pre_rows(qpd_decoder *d, const uint32_t *rows, int64_t Bc, uint8_t *out, hipStream_t st) {
    qpd::FastPlan fp = d->fplan;
    fp.in_vec = 1;
    fp.in_shift = fp.n - 2;
    if (d->pfx[0].nops > 0) {  // the frozen-prefix stages, then the decode
        int rc = QPD_OK;
        for (auto &sg : d->pfx)
            if (!rc && sg.nops > 0) rc = ensure_records(sg.buf, sg.cap, Bc, sg.rec, sg.paths);
        if (!rc) rc = patch_imports(d, st);
        if (rc) return rc;
        qpd::FastPlan pp = fp;
        const qpd::MOp *ops = (const qpd::MOp *)d->pfx_mops.p;
        for (const auto &sg : d->pfx) {  // each stage with ops: `paths` lanes and list entries per frame
            if (sg.nops > 0) {
                const int ps = __builtin_ctz(sg.paths);
                pp.ops = ops;
                pp.nops = sg.nops;
                pp.gs = pp.L = sg.paths;
                pp.fpw = 64 >> ps;
                pp.pfx = (uint32_t *)sg.buf.p;
                pp.pfx_rec = sg.rec;
                pp.pfx_geo = prefix_geo(ps);
                pp.pm_off = sg.pm;
                if ((rc = fast_launch(d, pp, (const int32_t *)rows, Bc, nullptr, st, true))) return rc;
            }
            ops += sg.nops;
        }
    }
    return fast_launch(d, fp, (const int32_t *)rows, Bc, out, st);
}

// Pre-pass rows (N bytes per frame) for up to d->pre_chunk of B frames: the
// frames per chunk.
int64_t reserve_pre_rows(qpd_decoder *d, int64_t B, int *rc) {
    return d->pre_rows.reserve(std::min<int64_t>(B, d->pre_chunk), (size_t)d->N, "pre-pass rows hipMalloc: ", rc);
}

// int32 symbols of at most `lim` of B frames, or 1 GB of them (2^18 frames at
// N = 1024), in a staging buffer: the frames per chunk.
int64_t reserve_symbols(qpd_decoder *d, DeviceChunk &buf, int64_t B, int64_t lim, const char *what, int *rc) {
    if (!lim) lim = std::max<int64_t>(1, ((int64_t)1 << 30) / ((int64_t)d->N * 4));
    return buf.reserve(std::min<int64_t>(B, lim), (size_t)d->N * sizeof(int32_t), what, rc);
}

// Pre-mode: the root pre-pass on the channel symbols (int32, or uint8 read as
// they are), then the decode on its rows, chunk by chunk.  fp.in_vec: the
// symbol rows allow the reader's vector loads (chan_word8).
template <class In>
int decode_pre_mode(qpd_decoder *d, qpd::FastPlan fp, const In *d_symbols, int64_t B, uint8_t *d_out, hipStream_t st) {
    int rc = QPD_OK;
    const int64_t chunk = reserve_pre_rows(d, B, &rc);
    if (rc) return rc;
    uint32_t *pre = (uint32_t *)d->pre_rows.p;
    for (int64_t f0 = 0; f0 < B; f0 += chunk) {
        int64_t Bc = std::min<int64_t>(chunk, B - f0);
        const In *sym = d_symbols + f0 * fp.N;
        fp.in_shift = fp.n;
        const int pgrid = (int)std::min<int64_t>(((Bc << (fp.n - 4)) + 255) / 256, 8192);
        void *pargs[] = {&fp, &sym, &Bc, &pre};
        rc = timed_launch(d, QPD_KC_PRE, st, [&]() -> int {
            const void *pk = d->row_lo ? reinterpret_cast<const void *>(&qpd::root_pre_kernel<In, true>)
                                       : reinterpret_cast<const void *>(&qpd::root_pre_kernel<In, false>);
            QPD_HIP(hipLaunchKernel(pk, dim3(pgrid), dim3(256), pargs, 0, st));
            QPD_HIP(hipGetLastError());
            return QPD_OK;
        });
        if (rc) return rc;
        rc = decode_pre_rows(d, pre, Bc, d_out + f0 * fp.out_k, st);
        if (rc) return rc;
    }
    return QPD_OK;
}

int decode_impl(qpd_decoder *d, const int32_t *d_symbols, int64_t B, uint8_t *d_out, hipStream_t st) {
    d->last_engine = QPD_RAN_GPU;
    d->u8_staged = 0;
    if (d->engine != QPD_ENGINE_FAST) {
        const int64_t groups = (B + d->plan.fpw - 1) / d->plan.fpw;
        return launch_generic(d, d_symbols, B, d_out, (int)std::min<int64_t>(groups, d->max_waves), st);
    }
    qpd::FastPlan fp = d->fplan;
    fp.in_vec = ((uintptr_t)d_symbols & 15u) == 0 && (fp.N & 3) == 0;
    if (!d->pre) {
        fp.in_shift = fp.n;
        return fast_launch(d, fp, d_symbols, B, d_out, st);
    }
    return decode_pre_mode(d, fp, d_symbols, B, d_out, st);
}

// uint8 channel symbols (caller: lock held, stream ordered).  Pre-mode reads
// them as they are (root_pre_kernel<uint8_t>); everything else widens a chunk
// into the int32 staging buffer on the same stream and runs the int32 launch.
int decode_u8_impl(qpd_decoder *d, const uint8_t *d_symbols, int64_t B, uint8_t *d_out, hipStream_t st) {
    if (d->engine == QPD_ENGINE_FAST && d->pre) {
        d->last_engine = QPD_RAN_GPU;
        d->u8_staged = 0;
        qpd::FastPlan fp = d->fplan;
        fp.in_vec = ((uintptr_t)d_symbols & 7u) == 0;  // N >= 16: every row and half keeps the base's alignment
        return decode_pre_mode(d, fp, d_symbols, B, d_out, st);
    }
    int rc = QPD_OK;
    const int64_t chunk = reserve_symbols(d, d->u8_sym, B, d->u8_chunk, "uint8 staging hipMalloc: ", &rc);
    if (rc) return rc;
    int32_t *stage = (int32_t *)d->u8_sym.p;
    for (int64_t f0 = 0; f0 < B; f0 += chunk) {
        const int64_t Bc = std::min<int64_t>(chunk, B - f0);
        const int64_t n = Bc * d->N;
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((n / 4 + 255) / 256, 8192));
        hipLaunchKernelGGL(qpd::widen_u8_kernel, dim3(grid), dim3(256), 0, st, d_symbols + f0 * d->N, n, stage);
        QPD_HIP(hipGetLastError());
        if ((rc = decode_impl(d, stage, Bc, d_out + f0 * d->out_bits, st))) return rc;
    }
    d->u8_staged = 1;
    return QPD_OK;
}

// d_metric: NULL, or qpd_dmetric's output (then d_out may be NULL).
int decode_f64_impl(qpd_decoder *d, const double *d_llr, int64_t B, uint8_t *d_out, hipStream_t st,
                    double *d_metric = nullptr) {
    d->last_engine = QPD_RAN_GPU;
    d->u8_staged = 0;
    const int64_t groups = (B + d->plan.fpw - 1) / d->plan.fpw;
    const int grid = (int)std::min<int64_t>(groups, d->max_waves);
    return launch_generic(d, d_llr, B, d_out, grid, st, d_metric);
}

// The checks the decode entry points share.  *run = false where there is
// nothing to decode (a refusal, or an empty batch: QPD_OK).  lut: the entry
// point takes LUT symbols (qpd_decode, qpd_decode_u8), not LLRs
// (qpd_decode_f64); suffix: "" or, for the host-buffer entry points, "_host".
int check_decode_args(const qpd_decoder *d, bool lut, const char *suffix, int64_t B, const void *in, const void *out,
                      bool *run) {
    *run = false;
    if (!d) return fail(QPD_E_INVALID, "null decoder");
    if (lut != (d->dom == qpd::DOM_LUT))
        return fail(QPD_E_INVALID, std::string(lut ? "this decoder takes float64 LLRs: use qpd_decode_f64"
                                                   : "LUT decoders take int32 channel symbols: use qpd_decode") + suffix);
    if (B < 0) return fail(QPD_E_INVALID, "negative batch");
    if (B == 0) return QPD_OK;
    if (!in || !out) return fail(QPD_E_INVALID, "null buffer");
    *run = true;
    return QPD_OK;
}

// One device-buffer decode by input type (qpd_decode_status; caller as above).
int decode_typed(qpd_decoder *d, const void *d_in, int32_t in_type, int64_t B, uint8_t *d_out, hipStream_t st) {
    switch (in_type) {
        case QPD_IN_I32: return decode_impl(d, (const int32_t *)d_in, B, d_out, st);
        case QPD_IN_U8: return decode_u8_impl(d, (const uint8_t *)d_in, B, d_out, st);
        default: return decode_f64_impl(d, (const double *)d_in, B, d_out, st);
    }
}

// The status request of a call, held by the handle while its launches are made.
struct StatusScope {
    qpd_decoder *d;
    StatusScope(qpd_decoder *d_, const qpd_stat::Req &rq, const uint8_t *out0) : d(d_) {
        d->st_req = rq;
        d->st_out0 = out0;
    }
    ~StatusScope() {
        d->st_req = qpd_stat::Req();
        d->st_out0 = nullptr;
    }
};

// The search request of a call, likewise (the call's d_out, or ls_out when it gave none), and
// its set made resident: a set that differs from the resident one is uploaded on the
// decoder's own stream, after the decoder's previous work (which may still read the old
// set), and waited for, so that every launch of the call, on any stream, finds it.
struct SearchScope {
    qpd_decoder *d;
    int rc = QPD_OK;
    SearchScope(qpd_decoder *d_, const qpd_search::Req &rq, const uint8_t *out0) : d(d_) {
        d->sr_req = rq;
        d->st_out0 = out0;
        rc = upload_set();
    }
    int upload_set() {
        if (!d->sr_set.p) {
            QPD_HIP(hipMalloc(&d->sr_set.p, QPD_MAX_SEARCH_MASKS * sizeof(uint32_t)));
            d->sr_set_host.clear();
        } else if (d->sr_set_host == d->sr_req.words) {
            return QPD_OK;
        }
        d->sr_set_host.clear();  // (nothing resident, should the upload fail)
        if (d->sr_req.words.empty()) return QPD_OK;
        const int orc = order_on(d, d->hs);
        if (orc) return orc;
        QPD_HIP(hipMemcpyAsync(d->sr_set.p, d->sr_req.words.data(), d->sr_req.words.size() * sizeof(uint32_t),
                               hipMemcpyHostToDevice, d->hs));
        QPD_HIP(hipStreamSynchronize(d->hs));
        d->sr_set_host = d->sr_req.words;
        return QPD_OK;
    }
    ~SearchScope() {
        d->sr_req = qpd_search::Req();
        d->st_out0 = nullptr;
    }
};

// The list request of a call, likewise.
struct ListScope {
    qpd_decoder *d;
    ListScope(qpd_decoder *d_, const qpd_list::Req &rq, const uint8_t *out0) : d(d_) {
        d->ls_req = rq;
        d->st_out0 = out0;
    }
    ~ListScope() {
        d->ls_req = qpd_list::Req();
        d->st_out0 = nullptr;
    }
};

}  // namespace
