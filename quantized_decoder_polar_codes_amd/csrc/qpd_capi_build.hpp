// qpd_capi_build.hpp -- the steps of qpd_create after validation: the handle's
// fields and engine, the generic engine's plan, the table uploads, the scratch,
// the fast engine's plan made resident (build_fast), the host engine
// (build_host).  Host code; the decisions themselves are qpd_config.hpp's and
// qpd_plan.hpp's.
#pragma once
#include <cstdlib>
#include <cstring>
#include <map>

#include "qpd_config.hpp"
#include "qpd_decoder.hpp"
#include "qpd_plan.hpp"
#include "qpd_schedule.hpp"

// Kernel instantiations, each in its own translation unit (build.py UNITS:
// the units compile in parallel).
namespace qpd {
const void *fast_kernel_single(int kind, int sets);              // qpd_k_fast.hip
const void *prefix_kernel(int kind, int sets, bool pw1);         // qpd_k_fast.hip
const void *fast_kernel_scl(int sets, bool l8, bool w16);        // qpd_k_scl.hip
const void *fast_kernel_scl_pw1(int sets, bool l8, bool w16);    // qpd_k_scl1.hip
const void *fast_kernel_fscl(int sets, bool l8, bool r1l);       // qpd_fast_fscl.hip
const void *fast_kernel_fscl_pw1(int sets, bool l8, bool r1l);   // qpd_fast_fscl1.hip
const void *fast_kernel_fscl_w16(int sets, bool pw1);            // qpd_fast_fscl16.hip
const void *generic_kernel(int fam, int dom, bool wide);         // qpd_k_generic.hip
const void *generic_list_kernel(int fam, int dom, bool wide);    // qpd_k_generic_ls.hip: list kinds + list output
const void *dmetric_kernel();                                    // qpd_k_generic_dm.hip: float FastSC + D-metric
// the list kinds' decode-status instantiations (ST), one unit per unit above (*_st.hip)
const void *fast_kernel_scl_st(int sets, bool l8, bool w16);
const void *fast_kernel_scl_pw1_st(int sets, bool l8, bool w16);
const void *fast_kernel_fscl_st(int sets, bool l8, bool r1l);
const void *fast_kernel_fscl_pw1_st(int sets, bool l8, bool r1l);
const void *fast_kernel_fscl_w16_st(int sets, bool pw1);
// ... and their list-output instantiations (LIST, the *_ls.hip units)
const void *fast_kernel_scl_ls(int sets, bool l8, bool w16);
const void *fast_kernel_scl_pw1_ls(int sets, bool l8, bool w16);
const void *fast_kernel_fscl_ls(int sets, bool l8, bool r1l);
const void *fast_kernel_fscl_pw1_ls(int sets, bool l8, bool r1l);
const void *fast_kernel_fscl_w16_ls(int sets, bool pw1);
}  // namespace qpd

namespace {

using qpd_sched::Schedule;

// The decode kernel instantiation of a plan (nullptr: none, the launch fails).
// pw1: the op list's pointer fields fit one word (compact_pointer_fields).
// st: 0 the plain kernel, 1 its ST twin, 2 its LIST twin.
const void *fast_kernel(int kind, int sets, bool l8, bool r1l, bool pw1, bool w16, int st = 0) {
    if (st == 2) {  // the same plan's kernel with the list-output tail (list kinds)
        switch (kind) {
            case QPD_SCL_LUT:
                return r1l ? nullptr : pw1 ? qpd::fast_kernel_scl_pw1_ls(sets, l8, w16) : qpd::fast_kernel_scl_ls(sets, l8, w16);
            case QPD_FASTSCL_LUT:
                if (w16) return r1l ? nullptr : qpd::fast_kernel_fscl_w16_ls(sets, pw1);
                return pw1 ? qpd::fast_kernel_fscl_pw1_ls(sets, l8, r1l) : qpd::fast_kernel_fscl_ls(sets, l8, r1l);
            default: return nullptr;
        }
    }
    if (st) {  // the same plan's kernel with the decode-status tail (list kinds)
        switch (kind) {
            case QPD_SCL_LUT:
                return r1l ? nullptr : pw1 ? qpd::fast_kernel_scl_pw1_st(sets, l8, w16) : qpd::fast_kernel_scl_st(sets, l8, w16);
            case QPD_FASTSCL_LUT:
                if (w16) return r1l ? nullptr : qpd::fast_kernel_fscl_w16_st(sets, pw1);
                return pw1 ? qpd::fast_kernel_fscl_pw1_st(sets, l8, r1l) : qpd::fast_kernel_fscl_st(sets, l8, r1l);
            default: return nullptr;
        }
    }
    switch (kind) {
        case QPD_SC_LUT:
        case QPD_FASTSC_LUT: return pw1 || r1l ? nullptr : qpd::fast_kernel_single(kind, sets);
        case QPD_SCL_LUT: return r1l ? nullptr : pw1 ? qpd::fast_kernel_scl_pw1(sets, l8, w16) : qpd::fast_kernel_scl(sets, l8, w16);
        case QPD_FASTSCL_LUT:
            if (w16) return r1l ? nullptr : qpd::fast_kernel_fscl_w16(sets, pw1);
            return pw1 ? qpd::fast_kernel_fscl_pw1(sets, l8, r1l) : qpd::fast_kernel_fscl(sets, l8, r1l);
        default: return nullptr;
    }
}
using qpd::generic_kernel;
using qpd::prefix_kernel;

// Task queue of the persistent kernels: one counter, never reset (wave_take).
// QPD_TASK_BASE0 (tests only) starts it elsewhere, e.g. just below 2^32 so
// that the first launches wrap around.
int init_task_queue(qpd_decoder *d) {
    uint32_t v0 = 0;
    if (const char *e = getenv("QPD_TASK_BASE0")) v0 = (uint32_t)strtoull(e, nullptr, 0);
    const uint32_t init[2] = {v0, 0u};
    const int rc = upload(d->task_ctr, init, 2, d->hs);
    if (rc) return rc;
    d->task_base = v0;
    return QPD_OK;
}

#ifdef QPD_STAMPS
// Diagnostic builds: the per-op-class cycle accumulators every decoder's
// kernels add to (qpd_debug_stamps), one device buffer per device (qpd_debug_stamps reads the
// current device's).
unsigned long long *stamp_buffer() {  // one per device (the current one)
    static std::mutex mu;
    static std::map<int, unsigned long long *> bufs;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lk(mu);
    unsigned long long *&buf = bufs[dev];
    if (!buf && hipMalloc(&buf, 64 * sizeof(unsigned long long)) == hipSuccess)
        (void)hipMemset(buf, 0, 64 * sizeof(unsigned long long));
    return buf;
}
#endif

// The kernel must declare no static LDS: the byte tables occupy the first
// 768 B of the wave's dynamic LDS (the rows and the selection scratch come
// after them), and their lookups address LDS offset 0 as the start of the
// dynamic allocation (qpd_fast_lookup.hpp lut_lds).
int check_no_static_lds(const void *kfn, const char *what) {
    hipFuncAttributes fa;
    QPD_HIP(hipFuncGetAttributes(&fa, kfn));
    if (fa.sharedSizeBytes != 0) return fail(QPD_E_DEVICE, std::string(what) + " declares static LDS");
    return QPD_OK;
}

// The handle's fields that follow from the configuration alone, and its
// engine.  cfg: as the caller passed it; fam, n, dom: validate's.
int configure(qpd_decoder *d, const qpd_config *cfg, int fam, int n, int dom) {
    const bool ca = qpd_sched::is_ca(cfg->kind);
    d->pub_kind = cfg->kind;
    d->dom = dom;
    d->out_bits = ca ? cfg->A : cfg->K;
    if (ca) {
        d->ca_A = cfg->A;
        d->crc_n = cfg->crc_n;
        d->crc_q = qpd_cfg::crc_taps(cfg->crc_n, cfg->crc_loc, cfg->crc_loc_count);
    }
    d->kind = fam;
    d->N = cfg->N;
    d->n = n;
    d->K = cfg->K;
    const bool list = fam == QPD_SCL_LUT || fam == QPD_FASTSCL_LUT;
    d->L = list ? cfg->L : 1;
    d->v = (dom == qpd::DOM_LUT || dom == qpd::DOM_UNIFORM) ? cfg->v : 0;
    d->device = cfg->device;
    int want = cfg->engine;
    if (const char *e = getenv("QPD_ENGINE")) want = atoi(e);
    std::string err;
    const int engine = qpd_cfg::choose_engine(dom, cfg->f_step, cfg->g_step, cfg->v, fam, d->L, want, err);
    if (engine < 0) return fail(engine, err);
    d->engine = engine;
    if (const char *e = getenv("QPD_U8_CHUNK")) d->u8_chunk = std::max<int64_t>(1, atoll(e));
    if (const char *e = getenv("QPD_LLR_COOP")) d->llr_coop = atoi(e) != 0;
    return QPD_OK;
}

// The generic engine's plan without its device pointers: sizes, the scratch
// rows (qpd_config.hpp: generic_layout) and the waves its scratch allows.
void plan_generic(qpd_decoder *d, const qpd_config *c, const Schedule &s) {
    DevPlan &P = d->plan;
    P.N = c->N;
    P.n = d->n;
    P.K = c->K;
    P.L = d->L;
    P.v = d->v;
    int gs = 1;
    while (gs < d->L) gs *= 2;
    P.gs = gs;
    P.fpw = 64 / gs;
    P.nops = (int)s.ops.size();
    P.max_r1 = s.max_r1;
    const qpd_cfg::GenericLayout G = qpd_cfg::generic_layout(d->kind, d->dom, c->N, d->n, s.max_r1);
    std::memcpy(P.So, G.So, sizeof P.So);
    std::memcpy(P.Uo, G.Uo, sizeof P.Uo);
    P.Ro = G.Ro;
    P.Ho = G.Ho;
    P.Ko = G.Ko;
    P.Io = G.Io;
    P.rows_per_wave = G.rows_per_wave;
    P.f_step = c->f_step;
    P.g_step = c->g_step;
    d->scratch_bytes_per_wave = (int64_t)G.rows_per_wave * 64 * 4;
    int mw = c->max_waves > 0 ? c->max_waves : 256 * 8;
    const int64_t cap = (int64_t)2 << 30;  // <= 2 GiB of scratch
    mw = (int)std::max<int64_t>(1, std::min<int64_t>(mw, cap / d->scratch_bytes_per_wave));
    d->max_waves = mw;
}

// The schedule, the information positions and the tables of the symbol domain.
int upload_tables(qpd_decoder *d, const qpd_config *c, const Schedule &s) {
    const int N = c->N;
    int rc;
    std::vector<int32_t> info;
    for (int i = 0; i < N; ++i)
        if (c->frozen_bits[i] == 0) info.push_back(i);
    std::vector<uint32_t> mask((N + 31) / 32, 0u);
    for (int i : info) mask[i >> 5] |= 1u << (i & 31);
    if ((rc = upload(d->ops, s.ops.data(), s.ops.size(), d->hs))) return rc;
    if ((rc = upload(d->info_pos, info.data(), info.size(), d->hs))) return rc;
    if ((rc = upload(d->info_mask, mask.data(), mask.size(), d->hs))) return rc;
    if (d->dom == qpd::DOM_UNIFORM) {
        if ((rc = upload(d->r_f, c->r_f, (size_t)N - 1, d->hs))) return rc;
        if ((rc = upload(d->r_g, c->r_g, (size_t)N - 1, d->hs))) return rc;
    } else if (d->dom == qpd::DOM_LLOYD) {
        if ((rc = upload(d->q_bnd, c->q_bnd, (size_t)c->q_bnd_count, d->hs))) return rc;
        if ((rc = upload(d->q_rec, c->q_rec, (size_t)c->q_rec_count, d->hs))) return rc;
        if ((rc = upload(d->bnd_off, c->bnd_off, 2 * ((size_t)N - 1), d->hs))) return rc;
        if ((rc = upload(d->bnd_len, c->bnd_len, 2 * ((size_t)N - 1), d->hs))) return rc;
        if ((rc = upload(d->rec_off, c->rec_off, 2 * ((size_t)N - 1), d->hs))) return rc;
        if ((rc = upload(d->rec_len, c->rec_len, 2 * ((size_t)N - 1), d->hs))) return rc;
    }
    if (d->dom == qpd::DOM_LUT) {
        const size_t vv = (size_t)c->v * c->v;
        if ((rc = upload(d->lut_f, c->lut_f, (size_t)c->lut_f_count * vv, d->hs))) return rc;
        if ((rc = upload(d->lut_g, c->lut_g, (size_t)c->lut_g_count * 2 * vv, d->hs))) return rc;
        if ((rc = upload(d->f_base, c->f_base, (size_t)N - 1, d->hs))) return rc;
        if ((rc = upload(d->g_base, c->g_base, (size_t)N - 1, d->hs))) return rc;
        if ((rc = upload(d->vcl, c->vcl, (size_t)c->vcl_rows * N * c->v, d->hs))) return rc;
    }
    return QPD_OK;
}

// The generic engine's scratch (the fast engine allocates its own slab in
// build_fast) and the error word, cleared.
int alloc_scratch(qpd_decoder *d) {
    hipError_t e = hipSuccess;
    if (d->engine == QPD_ENGINE_GENERIC) e = hipMalloc(&d->scratch.p, (size_t)d->scratch_bytes_per_wave * d->max_waves);
    if (e != hipSuccess) return fail(QPD_E_DEVICE, std::string("scratch hipMalloc: ") + hipGetErrorString(e));
    e = hipMalloc(&d->err.p, sizeof(int32_t));
    if (e == hipSuccess) e = hipMemsetAsync(d->err.p, 0, sizeof(int32_t), d->hs);
    if (e == hipSuccess) e = hipStreamSynchronize(d->hs);
    if (e != hipSuccess) return fail(QPD_E_DEVICE, std::string("err hipMalloc: ") + hipGetErrorString(e));
    return QPD_OK;
}

// The host plan's sizes, rows and kernel variant, copied to the handle and its FastPlan.
void adopt_fast_plan(qpd_decoder *d, const qpd_config *c, const Schedule &s, const qpd_plan::FastHostPlan &H) {
    qpd::FastPlan &F = d->fplan;
    F.N = c->N;
    F.n = d->n;
    F.K = c->K;
    F.L = d->L;
    F.v = c->v;
    F.gs = d->plan.gs;
    F.fpw = d->plan.fpw;
    F.max_r1 = s.max_r1;
    F.lds_from = H.lds_from;
    F.lds_rows = H.lds_rows;
    F.glb_rows = H.glb_rows;
    F.R0_row = H.R0_row;
    F.R0_lds = H.R0_lds;
    F.H_row = H.H_row;
    F.K_row = H.K_row;
    F.I_row = H.I_row;
    d->lds_bytes = H.lds_bytes;
    d->lds_tab_bytes = H.lds_tab_bytes;
    d->sets = H.sets;
    d->pfx_sets = H.pfx_sets;
    d->l8 = H.l8;
    d->w16 = H.w16;
    d->r1l = H.r1l;
    d->pw1 = H.pw1;
    d->pre = H.pre;
    d->row_lo = H.row_lo;
    d->pre_chunk = H.pre_chunk;
    for (int i = 0; i < 3; ++i) {
        d->pfx[i].nops = (int)H.pfx[i].size();
        d->pfx[i].rec = H.pfx_rec[i], d->pfx[i].pm = H.pfx_pm[i];
        d->pfx[i].paths = 1 << i;  // 1, 2, 4
    }
    F.nops = (int)H.ops.size();
    d->num_mops = F.nops + d->prefix_ops();
}

// The host plan's tables and op lists on the device.
int upload_fast_plan(qpd_decoder *d, const qpd_plan::FastHostPlan &H) {
    int rc;
    if ((rc = upload(d->r1_rank, H.r1tab.data(), H.r1tab.size(), d->hs))) return rc;
    for (const auto &st : H.pfx)  // one device array: stage 1, stage 1b, then stage 2
        d->pfx_ops_host.insert(d->pfx_ops_host.end(), st.begin(), st.end());
    if (!d->pfx_ops_host.empty()) {
        if ((rc = upload(d->pfx_mops, d->pfx_ops_host.data(), d->pfx_ops_host.size(), d->hs))) return rc;
        d->main_ops_host = H.ops;  // the import ops get the record buffers' addresses (patch_imports)
    }
    if ((rc = upload(d->mops, H.ops.data(), H.ops.size(), d->hs))) return rc;
    if ((rc = upload(d->f_tab, H.ft.data(), H.ft.size(), d->hs))) return rc;
    return upload(d->g_tab, H.gt.data(), H.gt.size(), d->hs);
}

// The fast engine's plan (qpd_plan.hpp: plan_fast), made resident on the device.
int build_fast(qpd_decoder *d, const qpd_config *c, const Schedule &s) {
    qpd::FastPlan &F = d->fplan;
#ifdef QPD_STAMPS
    F.stamps = stamp_buffer();
#endif
    qpd_plan::FastHostPlan H;
    std::string err;
    int rc = qpd_plan::plan_fast(*c, d->n, d->L, s, qpd_plan::PlanSwitches::from_env(), H, err);
    if (rc) return fail(rc, err);
    adopt_fast_plan(d, c, s, H);
    if ((rc = upload_fast_plan(d, H))) return rc;
    const void *kfn = fast_kernel(d->kind, d->sets, d->l8, d->r1l, d->pw1, d->w16);
    if (!kfn) return fail(QPD_E_UNSUPPORTED, "fast plan: no decode kernel instantiation for this plan");
    if ((rc = check_no_static_lds(kfn, "fast decode kernel"))) return rc;
    if (d->kind == QPD_SCL_LUT || d->kind == QPD_FASTSCL_LUT) {  // qpd_decode_status runs the plan's ST twin
        const void *ksfn = fast_kernel(d->kind, d->sets, d->l8, d->r1l, d->pw1, d->w16, 1);
        if (!ksfn) return fail(QPD_E_UNSUPPORTED, "fast plan: no decode-status kernel instantiation for this plan");
        if ((rc = check_no_static_lds(ksfn, "fast decode-status kernel"))) return rc;
        if (d->L > 1 && d->L <= qpd_list::kMaxListOut) {  // ... and qpd_decode_list its LIST twin
            const void *klfn = fast_kernel(d->kind, d->sets, d->l8, d->r1l, d->pw1, d->w16, 2);
            if (!klfn) return fail(QPD_E_UNSUPPORTED, "fast plan: no list-output kernel instantiation for this plan");
            if ((rc = check_no_static_lds(klfn, "fast list-output kernel"))) return rc;
        }
    }
    // (the prefix stages' two-set instantiations do the same offset-0 byte-table lookups)
    if (d->pfx[0].nops > 0 && d->pfx_sets == 2 &&
        (rc = check_no_static_lds(prefix_kernel(d->kind, d->pfx_sets, d->pw1), "fast prefix kernel")))
        return rc;
    // Persistent grid: as many waves as can be resident at once.
    const int64_t per_wave = (int64_t)d->sets * F.glb_rows * 64 * 4;
    int mw = c->max_waves;
    if (mw <= 0) {
        int per_cu = 0;
        const int ncu = device_cus();
        const hipError_t oe = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kfn, 64, d->lds_bytes);
        if (oe != hipSuccess || per_cu <= 0) per_cu = 16;
        mw = std::max(1, ncu) * per_cu;
    }
    mw = (int)std::max<int64_t>(1, std::min<int64_t>(mw, ((int64_t)2 << 30) / per_wave));
    d->max_waves = mw;
    d->scratch_bytes_per_wave = per_wave;
    QPD_HIP(hipMalloc(&d->fscratch.p, (size_t)per_wave * mw));
    F.r1_rank = (const uint16_t *)d->r1_rank.p;
    F.f_tab = (const uint32_t *)d->f_tab.p;
    F.g_tab = (const uint32_t *)d->g_tab.p;
    F.vcl = (const double *)d->vcl.p;
    F.ops = (const qpd::MOp *)d->mops.p;
    F.info_pos = (const int32_t *)d->info_pos.p;
    F.scratch = (uint32_t *)d->fscratch.p;
    F.err = (int32_t *)d->err.p;
    if ((rc = init_task_queue(d))) return rc;
    F.task_ctr = (uint32_t *)d->task_ctr.p;
    return QPD_OK;
}

// The device pointers and the output epilogue's fields of both plans; the
// task queue, where build_fast has not made it.
int fill_plan_pointers(qpd_decoder *d) {
    DevPlan &P = d->plan;
    P.lut_f = (const uint8_t *)d->lut_f.p;
    P.f_base = (const int32_t *)d->f_base.p;
    P.lut_g = (const uint8_t *)d->lut_g.p;
    P.g_base = (const int32_t *)d->g_base.p;
    P.vcl = (const double *)d->vcl.p;
    P.ops = (const Op *)d->ops.p;
    P.info_pos = (const int32_t *)d->info_pos.p;
    P.scratch = (uint32_t *)d->scratch.p;
    P.err = (int32_t *)d->err.p;
    if (!d->task_ctr.p) {
        const int rc = init_task_queue(d);
        if (rc) return rc;
    }
    P.task_ctr = (uint32_t *)d->task_ctr.p;
    P.r_f = (const double *)d->r_f.p;
    P.r_g = (const double *)d->r_g.p;
    P.q_bnd = (const double *)d->q_bnd.p;
    P.q_rec = (const double *)d->q_rec.p;
    P.bnd_off = (const int32_t *)d->bnd_off.p;
    P.bnd_len = (const int32_t *)d->bnd_len.p;
    P.rec_off = (const int32_t *)d->rec_off.p;
    P.rec_len = (const int32_t *)d->rec_len.p;
    // DOUBLE_INF of each class: 1.0/0.0 for the LUT decoders and FastSCL
    // (SCLLUTDecoder.h:16, FastSCLDecoder.h:7), 1e300 for the float SCL family
    // (SCLDecoder.h:8, CASCLDecoder.h:9, SCL{Uniform,Lloyd}QuantizedDecoder.h)
    P.pm_init = (d->dom == qpd::DOM_LUT || d->kind == QPD_FASTSCL_LUT) ? __builtin_huge_val() : 1e300;
    P.out_k = d->out_bits;
    P.ca_A = d->ca_A;
    P.crc_n = d->crc_n;
    // bits compared after the A info bits: K - A (LUT kinds), crc_n (CASCLDecoder)
    P.ca_chk = d->pub_kind == QPD_CASCL_FLOAT ? d->crc_n : d->K - d->ca_A;
    P.crc_q = d->crc_q;
    P.info_mask = (const uint32_t *)d->info_mask.p;
    d->fplan.out_k = d->out_bits;
    d->fplan.ca_A = d->ca_A;
    d->fplan.crc_n = d->crc_n;
    d->fplan.crc_q = d->crc_q;
    d->fplan.info_mask = (const uint32_t *)d->info_mask.p;
    return QPD_OK;
}

// The host engine's copy of the plan (qpd_host.hpp) and the batch size up to
// which QPD_HOST_AUTO prefers it (qpd_config.hpp: host_max_frames).
int build_host(qpd_decoder *d, const qpd_config *cfg) {
    std::unique_ptr<qpd_host::Plan> h = qpd_host::make_plan(cfg);
    if (!h) return QPD_OK;  // re-quantized float kinds: GPU only
    if (h->dom == qpd::DOM_LUT)
        d->heng_lut = std::make_unique<qpd_host::Engine<uint8_t>>(*h);
    else
        d->heng_f64 = std::make_unique<qpd_host::Engine<double>>(*h);
    d->host_max_frames = qpd_cfg::host_max_frames(h->N, h->n, h->L);
    d->hplan = std::move(h);
    if (const char *e = getenv("QPD_HOST_ENGINE")) {
        if (!strcmp(e, "gpu")) d->host_mode = QPD_HOST_GPU;
        if (!strcmp(e, "cpu")) d->host_mode = QPD_HOST_CPU;
    }
    return QPD_OK;
}

// qpd_create after validation: the handle for `cfg` on the current device
// (cfg->device, selected by the caller, so that a failure's ~qpd_decoder
// frees there).  fam, n, dom: validate's.
int create_decoder(const qpd_config *cfg, int fam, int n, int dom, std::unique_ptr<qpd_decoder> &d) {
    // Every public kind is a kernel family in a symbol domain (family_of); the
    // CRC-aided kinds add an output epilogue.
    qpd_config cc = *cfg;
    cc.kind = fam;
    const qpd_config *c = &cc;
    d.reset(new qpd_decoder());
    const hipError_t e = hipStreamCreateWithFlags(&d->hs, hipStreamNonBlocking);
    if (e != hipSuccess) return fail(QPD_E_DEVICE, std::string("decoder stream: ") + hipGetErrorString(e));
    int rc;
    Schedule s;
    const bool fast_kind = fam == QPD_FASTSC_LUT || fam == QPD_FASTSCL_LUT;
    qpd_sched::visit(s, fam, c->N, n, c->frozen_bits, fast_kind ? c->node_type : nullptr, 0, 0);
    d->ops_host = s.ops;
    if ((rc = configure(d.get(), cfg, fam, n, dom))) return rc;
    plan_generic(d.get(), c, s);
    if ((rc = upload_tables(d.get(), c, s))) return rc;
    if ((rc = alloc_scratch(d.get()))) return rc;
    if (d->engine == QPD_ENGINE_FAST && (rc = build_fast(d.get(), c, s))) return rc;
    if ((rc = fill_plan_pointers(d.get()))) return rc;
    return build_host(d.get(), cfg);
}

}  // namespace
