// qpd_capi.hip -- C-ABI of libqpd.so (include/qpd.h): validation, device
// residency of the tables and plans (the traversal schedule: qpd_schedule.hpp,
// the fast engine's plan compiler: qpd_plan.hpp) and kernel launches.  Host
// code only; kernels in qpd_generic.hip / qpd_fast.hip and their units.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "qpd.h"
#include "qpd_generic.hip"
#include "qpd_fast_plan.hpp"
#include "qpd_fast_pre.hpp"

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
}  // namespace qpd
#include "qpd_mc.hip"
#include "qpd_probe.hip"
#include "qpd_host.hpp"
#include "qpd_plan.hpp"
#include "qpd_schedule.hpp"

#include <memory>

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

#define QPD_HIP(call)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess) return fail(QPD_E_DEVICE, std::string(#call ": ") + hipGetErrorString(e_)); \
    } while (0)

using qpd::DevPlan;
using qpd::Op;
using qpd_sched::Schedule;
using qpd_sched::special_of;
using qpd_sched::visit;
using qpd_sched::family_of;
using qpd_sched::is_ca;

int ilog2_exact(int N) {
    int n = 0;
    while ((1 << n) < N) ++n;
    return ((1 << n) == N) ? n : -1;
}

struct DeviceBuf {
    void *p = nullptr;
    ~DeviceBuf() {
        if (p) (void)hipFree(p);
    }
};

}  // namespace

struct qpd_decoder {
    int kind, N, n, K, L, v, device;  // kind: the kernel family (SC/SCL/FastSC/FastSCL LUT ids)
    int dom = 0;                      // qpd::Dom symbol domain
    int max_waves;
    int64_t scratch_bytes_per_wave;
    int engine = QPD_ENGINE_GENERIC;
    int lds_bytes = 0;
    int lds_tab_bytes = 0;  // of lds_bytes: the f / g ops' byte tables (SCL-LUT)
    int pub_kind = 0;  // the kind the caller asked for (CRC-aided kinds map to their list kind)
    int out_bits = 0;  // bits per decoded frame: K, or A for the CRC-aided kinds
    int ca_A = 0, crc_n = 0;
    uint32_t crc_q = 0;
    DeviceBuf info_mask;
    DeviceBuf mc_pref, mc_crc;  // qpd_mc_frames: info bits before each word; CRC contribution per message bit
    int sets = 1;  // fast engine: frame sets per wave (lut_fast_kernel NS)
    bool l8 = false;  // fast engine: list decoder with L = 8 (select_survivors8)
    bool w16 = false; // fast engine: SCL-LUT / FastSCL-LUT with 9 <= L <= 16 (lane groups of 16, select_survivors16)
    bool r1l = false;  // fast engine: an R1 node needs r1_large (the R1L instantiation)
    bool pw1 = false;  // fast engine: one pointer word per path (compact_pointer_fields)
    bool pre = false;         // fast engine pre-mode: root_pre_kernel, then the decode on its rows
    int64_t pre_chunk = 0;    // frames per pre-pass chunk
    int64_t pre_cap = 0;      // frames pre_buf holds
    bool pre_fell_back = false;  // an allocation of pre-pass rows failed: pre_cap is the chunk from then on
    DeviceBuf pre_buf;
    DeviceBuf mc_sym;        // qpd_mc_decode without a fused pre-pass: int32 symbols of one chunk
    int64_t mc_sym_cap = 0;  // frames mc_sym holds
    bool mc_sym_fell_back = false;
    DeviceBuf u8_sym;        // qpd_decode_u8 outside pre-mode: int32 symbols of one chunk (widen_u8_kernel)
    int64_t u8_cap = 0;      // frames u8_sym holds
    int64_t u8_chunk = 0;    // QPD_U8_CHUNK (tests): frames per staging chunk (0: 1 GB of int32 symbols)
    bool u8_fell_back = false;
    int u8_staged = 0;       // qpd_info.u8_staged: the last decode call widened its input into u8_sym
    DevPlan plan{};
    qpd::FastPlan fplan{};
    DeviceBuf f_tab, g_tab, fscratch, mops, r1_rank, task_ctr;
    int num_mops = 0;
    DeviceBuf pfx_mops;  // frozen-prefix stages' ops (lut_prefix_kernel): stage 1, stage 1b, then stage 2
    int pfx_sets = 1;    // frame sets per wave of the prefix stages (QPD_PFX_SETS)
    // The stages in FastHostPlan's order: 1 (one path per frame; no ops: no split), 1b (<= 2 live
    // paths; no ops: stage 2 resumes from stage 1), 2 (<= 4 live paths; no ops: the decode kernel
    // resumes from stage 1).
    struct PrefixStage {
        int nops = 0;          // the stage's ops in pfx_mops, after the earlier stages'
        int rec = 0, pm = 0;   // words per path record, metric word in it
        int paths = 1;         // paths per frame: the stage's list size and lanes per frame
        DeviceBuf buf;         // the stage's records (interleaved, see FastPlan::pfx)
        size_t cap = 0;
        const void *patched = nullptr;  // the buffer address the device copies of the import ops hold
    } pfx[3];
    int prefix_ops() const { return pfx[0].nops + pfx[1].nops + pfx[2].nops; }
    std::vector<qpd::MOp> pfx_ops_host, main_ops_host;  // host copies of the split schedule (patch_imports)
    std::vector<Op> ops_host;
    DeviceBuf lut_f, f_base, lut_g, g_base, vcl, ops, info_pos, scratch, err;
    DeviceBuf r_f, r_g, q_bnd, q_rec, bnd_off, bnd_len, rec_off, rec_len;  // float-domain re-quantizers
    // staging for the host-buffer entry points
    DeviceBuf h_in, h_out;
    size_t h_in_bytes = 0, h_out_bytes = 0;
    // The decoder's own stream (created with the handle): every upload of
    // qpd_create, the host-buffer entry points (pinned staging, one stream
    // synchronization per call: copy in, decode, copy out + error word) and
    // the error-word checks run on it.
    hipStream_t hs = nullptr;
    void *pin = nullptr;
    size_t pin_bytes = 0;
    // Ordering across streams (thread-safe per handle per
    // stream).  The work buffers (slab, pre-pass rows, task queue, error word,
    // staging) are per decoder, so every call first makes its stream wait for
    // the decoder's previous work when that ran on another stream
    // (hipStreamWaitEvent on `last_ev`), and records `last_ev` on its own
    // stream after its launches.  `mu` serializes host threads on one handle.
    std::mutex mu;
    hipEvent_t last_ev = nullptr;
    hipStream_t last_st = nullptr;
    bool last_valid = false;
    uint32_t task_base = 0;  // task queue counter at the start of the next launch (wave_take)
    // Host engine (qpd_host.hpp) for the host-buffer entry points' small
    // batches: the per-frame drop-in call.  Null for the kinds it does not
    // decode (re-quantized float domains).
    std::unique_ptr<qpd_host::Plan> hplan;
    std::unique_ptr<qpd_host::Engine<uint8_t>> heng_lut;
    std::unique_ptr<qpd_host::Engine<double>> heng_f64;
    int host_mode = QPD_HOST_AUTO;
    int64_t host_max_frames = 0;  // QPD_HOST_AUTO: batches up to this size run on the host engine
    int last_engine = QPD_RAN_NONE;  // what served the last decode call (qpd_info.last_engine)
    // qpd_profile: HIP events around every launch, per kernel class
    bool prof = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_ev[QPD_KC_COUNT];
    ~qpd_decoder() {
        if (last_valid) (void)hipEventSynchronize(last_ev);  // no buffer is freed under a running launch
        if (hs) (void)hipStreamSynchronize(hs);
        if (last_ev) (void)hipEventDestroy(last_ev);
        if (hs) (void)hipStreamDestroy(hs);
        if (pin) (void)hipHostFree(pin);
        for (auto &v : prof_ev)
            for (auto &e : v) {
                (void)hipEventDestroy(e.first);
                (void)hipEventDestroy(e.second);
            }
    }
};

namespace {

// Device copy of a host array on the decoder's own stream, complete on return
// (qpd_create: every table is resident before the handle is handed out, so no
// decode on any stream can overtake an upload).
template <class T>
int upload(DeviceBuf &b, const T *src, size_t count, hipStream_t st) {
    const size_t bytes = std::max<size_t>(1, count * sizeof(T));
    QPD_HIP(hipMalloc(&b.p, bytes));
    if (count) {
        QPD_HIP(hipMemcpyAsync(b.p, src, count * sizeof(T), hipMemcpyHostToDevice, st));
        QPD_HIP(hipStreamSynchronize(st));
    }
    return QPD_OK;
}

int set_device(const qpd_decoder *d) {
    if (d->device >= 0) QPD_HIP(hipSetDevice(d->device));
    return QPD_OK;
}

// Cross-stream ordering of one decoder's work (see qpd_decoder::last_ev):
// `order_on` before a call's first operation on stream st, `mark_on` after
// its last.
int order_on(qpd_decoder *d, hipStream_t st) {
    if (d->last_valid && d->last_st != st) QPD_HIP(hipStreamWaitEvent(st, d->last_ev, 0));
    return QPD_OK;
}

int mark_on(qpd_decoder *d, hipStream_t st) {
    if (!d->last_ev) QPD_HIP(hipEventCreateWithFlags(&d->last_ev, hipEventDisableTiming));
    QPD_HIP(hipEventRecord(d->last_ev, st));
    d->last_st = st;
    d->last_valid = true;
    return QPD_OK;
}

// One kernel launch of class kc on stream st; bracketed by HIP events on that
// stream while profiling is enabled (qpd_profile / qpd_kernel_times).
template <class F>
int timed_launch(qpd_decoder *d, int kc, hipStream_t st, F &&launch) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto drop = [&]() {  // no event outlives a failed record or launch
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    };
    if (d->prof) {
        hipError_t e = hipEventCreate(&e0);
        if (e == hipSuccess) e = hipEventCreate(&e1);
        if (e == hipSuccess) e = hipEventRecord(e0, st);
        if (e != hipSuccess) {
            drop();
            return fail(QPD_E_DEVICE, std::string("profiling event: ") + hipGetErrorString(e));
        }
    }
    const int rc = launch();
    if (d->prof) {
        const hipError_t e = rc ? hipSuccess : hipEventRecord(e1, st);
        if (rc || e != hipSuccess) {
            drop();
            return rc ? rc : fail(QPD_E_DEVICE, std::string("profiling event: ") + hipGetErrorString(e));
        }
        d->prof_ev[kc].emplace_back(e0, e1);
    }
    return rc;
}

// Kernel family (SC / SCL / FastSC / FastSCL, as the LUT kind ids) and symbol
// domain of every public kind; the CRC-aided kinds are their list family
// plus an output epilogue.
int validate(const qpd_config *c, int *n_out, int *fam_out, int *dom_out) {
    if (!c) return fail(QPD_E_INVALID, "null config");
    int fam = 0, dom = 0;
    if (!family_of(c->kind, &fam, &dom)) return fail(QPD_E_INVALID, "unknown decoder kind");
    if (is_ca(c->kind)) {
        if (c->crc_n < 1 || c->crc_n > 32) return fail(QPD_E_INVALID, "crc_n must be in [1, 32]");
        if (c->kind == QPD_CASCL_FLOAT) {
            // CASCLDecoder.cpp:218-226 compares crc_n bits after the A info bits:
            // A + crc_n > K would read past the decoded info bits (UB there).
            if (c->A < 1 || c->A + c->crc_n > c->K) return fail(QPD_E_INVALID, "CASCLDecoder needs 1 <= A and A + crc_n <= K");
        } else if (c->A < 1 || c->A > c->K || c->K - c->A > c->crc_n) {
            // CRC-aided LUT output (CASCLLUTDecoder.cpp:263-302): K - A > crc_n would
            // read past the reference's check code (UB there), so it is rejected here.
            return fail(QPD_E_INVALID, "CRC-aided kinds need 1 <= A <= K and K - A <= crc_n");
        }
        if (c->crc_loc_count < 0 || (c->crc_loc_count > 0 && !c->crc_loc)) return fail(QPD_E_INVALID, "bad crc_loc");
        for (int i = 0; i < c->crc_loc_count; ++i)
            if (c->crc_loc[i] < 0 || c->crc_loc[i] > c->crc_n) return fail(QPD_E_INVALID, "crc_loc entry outside [0, crc_n]");
    }
    const int n = ilog2_exact(c->N);
    if (c->N < 2 || n < 0 || n > qpd::kMaxDepth) return fail(QPD_E_INVALID, "N must be a power of two in [2, 65536]");
    if (!c->frozen_bits) return fail(QPD_E_INVALID, "frozen_bits is NULL");
    int zeros = 0;
    for (int i = 0; i < c->N; ++i) {
        if (c->frozen_bits[i] != 0 && c->frozen_bits[i] != 1)
            return fail(QPD_E_INVALID, "frozen_bits entries must be 0 or 1");
        zeros += c->frozen_bits[i] == 0;
    }
    if (zeros != c->K) return fail(QPD_E_INVALID, "K must equal the number of information (0) entries of frozen_bits");
    *n_out = n;
    *fam_out = fam;
    *dom_out = dom;
    const bool list = fam == QPD_SCL_LUT || fam == QPD_FASTSCL_LUT;
    if (list && (c->L < 1 || c->L > qpd::kMaxLWide))
        return fail(QPD_E_UNSUPPORTED, "list size L must be in [1, 32]");
    if (fam == QPD_FASTSC_LUT || fam == QPD_FASTSCL_LUT) {
        if (!c->node_type) return fail(QPD_E_INVALID, "node_type is required for the Fast decoders");
        if (special_of(fam, c->node_type, 0) >= 0)
            return fail(QPD_E_UNSUPPORTED, "root node labelled special (undefined behaviour in the reference)");
    }
    if (dom == qpd::DOM_UNIFORM && (!c->r_f || !c->r_g)) return fail(QPD_E_INVALID, "uniform kinds need r_f and r_g");
    if (dom == qpd::DOM_LLOYD) {
        if (!c->q_bnd || !c->q_rec || !c->bnd_off || !c->bnd_len || !c->rec_off || !c->rec_len)
            return fail(QPD_E_INVALID, "Lloyd kinds need boundary and reconstruction tables");
        for (int k = 0; k < 2 * (c->N - 1); ++k) {
            if (c->bnd_len[k] < 1 || c->bnd_off[k] < 0 || (long)c->bnd_off[k] + c->bnd_len[k] > c->q_bnd_count)
                return fail(QPD_E_INVALID, "Lloyd boundary list outside q_bnd (or empty)");
            if (c->rec_len[k] < 1 || c->rec_off[k] < 0 || (long)c->rec_off[k] + c->rec_len[k] > c->q_rec_count)
                return fail(QPD_E_INVALID, "Lloyd reconstruction list outside q_rec (or empty)");
        }
    }
    if (dom != qpd::DOM_LUT) return QPD_OK;
    if (c->v < 2 || c->v > 256) return fail(QPD_E_INVALID, "alphabet size v must be in [2, 256]");
    if (!c->lut_f || !c->lut_g || !c->f_base || !c->g_base || !c->vcl) return fail(QPD_E_INVALID, "null table pointer");
    if ((c->f_step != 0 && c->f_step != 1) || (c->g_step != 0 && c->g_step != 1))
        return fail(QPD_E_INVALID, "f_step/g_step must be 0 or 1");
    if (c->vcl_rows < n) return fail(QPD_E_INVALID, "vcl_rows must be >= log2(N)");
    const int vv = c->v * c->v;
    for (int p = 0; p < c->N - 1; ++p) {
        const int depth = 31 - __builtin_clz((unsigned)(p + 1));
        const int last = (c->N >> (depth + 1)) - 1;
        const long fl = (long)c->f_base[p] + (long)last * c->f_step;
        const long gl = (long)c->g_base[p] + (long)last * c->g_step;
        if (c->f_base[p] < 0 || fl >= c->lut_f_count) return fail(QPD_E_INVALID, "f_base/f_step index outside lut_f");
        if (c->g_base[p] < 0 || gl >= c->lut_g_count) return fail(QPD_E_INVALID, "g_base/g_step index outside lut_g");
    }
    for (long i = 0; i < (long)c->lut_f_count * vv; ++i)
        if (c->lut_f[i] >= c->v) return fail(QPD_E_INVALID, "lut_f entry outside [0, v)");
    for (long i = 0; i < (long)c->lut_g_count * 2 * vv; ++i)
        if (c->lut_g[i] >= c->v) return fail(QPD_E_INVALID, "lut_g entry outside [0, v)");
    for (long i = 0; i < (long)n * c->N * c->v; ++i)
        if (!std::isfinite(c->vcl[i])) return fail(QPD_E_INVALID, "vcl rows 0..n-1 must be finite");
    return QPD_OK;
}


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

// The decode kernel instantiation of a plan (nullptr: none, the launch fails).
// pw1: the op list's pointer fields fit one word (compact_pointer_fields).
const void *fast_kernel(int kind, int sets, bool l8, bool r1l, bool pw1, bool w16) {
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

// The kernel must declare no static LDS: the byte tables' lookups address LDS
// offset 0 as the start of the dynamic allocation (qpd_fast_lookup.hpp lut_lds).
int check_no_static_lds(const void *kfn, const char *what) {
    hipFuncAttributes fa;
    QPD_HIP(hipFuncGetAttributes(&fa, kfn));
    if (fa.sharedSizeBytes != 0) return fail(QPD_E_DEVICE, std::string(what) + " declares static LDS");
    return QPD_OK;
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
    d->pre_chunk = H.pre_chunk;
    for (int i = 0; i < 3; ++i) {
        d->pfx[i].nops = (int)H.pfx[i].size();
        d->pfx[i].rec = H.pfx_rec[i], d->pfx[i].pm = H.pfx_pm[i];
        d->pfx[i].paths = 1 << i;  // 1, 2, 4
    }
    F.nops = (int)H.ops.size();
    d->num_mops = F.nops + d->prefix_ops();
    if ((rc = upload(d->r1_rank, H.r1tab.data(), H.r1tab.size(), d->hs))) return rc;
    for (const auto &st : H.pfx)  // one device array: stage 1, stage 1b, then stage 2
        d->pfx_ops_host.insert(d->pfx_ops_host.end(), st.begin(), st.end());
    if (!d->pfx_ops_host.empty()) {
        if ((rc = upload(d->pfx_mops, d->pfx_ops_host.data(), d->pfx_ops_host.size(), d->hs))) return rc;
        d->main_ops_host = H.ops;  // the import ops get the record buffers' addresses (patch_imports)
    }
    if ((rc = upload(d->mops, H.ops.data(), H.ops.size(), d->hs))) return rc;
    if ((rc = upload(d->f_tab, H.ft.data(), H.ft.size(), d->hs))) return rc;
    if ((rc = upload(d->g_tab, H.gt.data(), H.gt.size(), d->hs))) return rc;
    const void *kfn = fast_kernel(d->kind, d->sets, d->l8, d->r1l, d->pw1, d->w16);
    if (!kfn) return fail(QPD_E_UNSUPPORTED, "fast plan: no decode kernel instantiation for this plan");
    if ((rc = check_no_static_lds(kfn, "fast decode kernel"))) return rc;
    // (the prefix stages' two-set instantiations do the same offset-0 byte-table lookups)
    if (d->pfx[0].nops > 0 && d->pfx_sets == 2 &&
        (rc = check_no_static_lds(prefix_kernel(d->kind, d->pfx_sets, d->pw1), "fast prefix kernel")))
        return rc;
    // Persistent grid: as many waves as can be resident at once.
    const int64_t per_wave = (int64_t)d->sets * F.glb_rows * 64 * 4;
    int mw = c->max_waves;
    if (mw <= 0) {
        int dev = 0, ncu = 256, per_cu = 0;
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
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


template <class In>
int launch_generic(qpd_decoder *d, const In *in, int64_t B, uint8_t *out, int grid, hipStream_t st) {
    const void *kfn = generic_kernel(d->kind, d->dom, d->L > qpd::kMaxL);
    if (!kfn) return fail(QPD_E_INVALID, "bad kind");
    qpd::DevPlan P = d->plan;
    P.task_base = d->task_base;
    const In *in_arg = in;
    void *args[] = {&P, &in_arg, &B, &out};
    const int rc = timed_launch(d, QPD_KC_DECODE, st, [&]() -> int {
        QPD_HIP(hipLaunchKernel(kfn, dim3(grid), dim3(64), args, 0, st));
        QPD_HIP(hipGetLastError());
        return QPD_OK;
    });
    if (!rc) d->task_base += (uint32_t)((B + d->plan.fpw - 1) / d->plan.fpw);  // takes of this launch (wave_take)
    return rc;
}

// The host engine's copy of the plan (qpd_host.hpp) and the batch size up to
// which QPD_HOST_AUTO prefers it.  The crossover is a cost model fitted to the
// per-call latencies measured on MI355X (tools/latency.py,
// profiles/r02_latency.jsonl, re-checked on profiles/r03af_latency.jsonl): a GPU call costs a fixed launch / copy /
// synchronization overhead plus one wave running the whole serial schedule,
// whatever the batch up to thousands of frames; the host engine costs its
// per-frame work times the batch.
int build_host(qpd_decoder *d, const qpd_config *cfg) {
    std::unique_ptr<qpd_host::Plan> h = qpd_host::make_plan(cfg);
    if (!h) return QPD_OK;  // re-quantized float kinds: GPU only
    if (h->dom == qpd::DOM_LUT)
        d->heng_lut = std::make_unique<qpd_host::Engine<uint8_t>>(*h);
    else
        d->heng_f64 = std::make_unique<qpd_host::Engine<double>>(*h);
    // Per frame on the host engine ~ its lookups (N log2 N per path) plus,
    // for lists, the forks (re-fitted to the round-3 engine, profiles/
    // r03af_latency.jsonl: SC-LUT N=128 2.8 us, N=1024 15.5 us, SCL-LUT
    // N=1024 L=8 0.154 ms); a GPU call ~ 55 us of launches, copies and
    // synchronization plus one wave running the serial schedule (SC-LUT N=128
    // 0.11 ms, N=1024 0.91 ms, SCL-LUT N=1024 L=8 1.07 ms, same file) -- flat
    // in the batch up to thousands of frames.
    const double nn = (double)h->N * h->n;
    const double host_us = 0.00136 * nn * h->L + (h->L > 1 ? 0.005 * h->L * h->N : 0.0) + 1.6;
    const double gpu_us = 55.0 + 0.083 * nn + (h->L > 1 ? 0.02 * nn : 0.0);
    d->host_max_frames = std::max<int64_t>(1, (int64_t)(gpu_us / host_us));
    d->hplan = std::move(h);
    if (const char *e = getenv("QPD_HOST_ENGINE")) {
        if (!strcmp(e, "gpu")) d->host_mode = QPD_HOST_GPU;
        if (!strcmp(e, "cpu")) d->host_mode = QPD_HOST_CPU;
    }
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
    int rc = validate(cfg, &n, &fam, &dom);
    if (rc) return rc;
    // Every public kind is a kernel family in a symbol domain (family_of); the
    // CRC-aided kinds add an output epilogue.
    qpd_config cc = *cfg;
    const bool ca = is_ca(cfg->kind);
    cc.kind = fam;
    const qpd_config *c = &cc;
    if (c->device >= 0) QPD_HIP(hipSetDevice(c->device));

    qpd_decoder *d = new qpd_decoder();
    {
        const hipError_t e = hipStreamCreateWithFlags(&d->hs, hipStreamNonBlocking);
        if (e != hipSuccess) {
            delete d;
            return fail(QPD_E_DEVICE, std::string("decoder stream: ") + hipGetErrorString(e));
        }
    }
    d->pub_kind = cfg->kind;
    d->dom = dom;
    d->out_bits = ca ? cfg->A : cfg->K;
    if (ca) {
        d->ca_A = cfg->A;
        d->crc_n = cfg->crc_n;
        for (int i = 0; i < cfg->crc_loc_count; ++i) {
            const int j = cfg->crc_loc[i];  // coefficient j -> register bit crc_n - j (j = 0: leading, drops out)
            if (j >= 1) d->crc_q |= 1u << (cfg->crc_n - j);
        }
    }
    d->kind = c->kind;
    d->N = c->N;
    d->n = n;
    d->K = c->K;
    const bool list = c->kind == QPD_SCL_LUT || c->kind == QPD_FASTSCL_LUT;
    d->L = list ? c->L : 1;
    d->v = (dom == qpd::DOM_LUT || dom == qpd::DOM_UNIFORM) ? c->v : 0;
    d->device = c->device;

    Schedule s;
    visit(s, c->kind, c->N, n, c->frozen_bits, (c->kind == QPD_FASTSC_LUT || c->kind == QPD_FASTSCL_LUT) ? c->node_type : nullptr, 0, 0);
    d->ops_host = s.ops;
    {
        // L > 8 (2L > 16: libstdc++ introsort, replayed where ties make it matter): up to L = 16 on
        // the fast engine (lane groups of 16, select_survivors16) -- SCL-LUT under AUTO, FastSCL-LUT
        // only on an explicit request (fast_avail): AUTO keeps it on the generic engine
        const bool fast_base = dom == qpd::DOM_LUT && c->f_step == 0 && c->g_step == 0 && c->v <= 16;
        const bool fast_auto = fast_base && (d->L <= qpd::kMaxL || (c->kind == QPD_SCL_LUT && d->L <= 2 * qpd::kMaxL));
        const bool fast_avail = fast_auto || (fast_base && c->kind == QPD_FASTSCL_LUT && d->L <= 2 * qpd::kMaxL);
        int want = c->engine;
        if (const char *e = getenv("QPD_ENGINE")) want = atoi(e);
        if (want == QPD_ENGINE_FAST && !fast_avail) {
            delete d;
            return fail(QPD_E_UNSUPPORTED,
                        "fast engine needs LUT symbols with one table per node (f_step = g_step = 0), v <= 16 and L <= 8 "
                        "(SCL-LUT and, on request, FastSCL-LUT: L <= 16)");
        }
        d->engine = want == QPD_ENGINE_FAST ? QPD_ENGINE_FAST
                    : (want == QPD_ENGINE_GENERIC || !fast_auto) ? QPD_ENGINE_GENERIC : QPD_ENGINE_FAST;
    }
    if (const char *e = getenv("QPD_U8_CHUNK")) d->u8_chunk = std::max<int64_t>(1, atoll(e));

    DevPlan &P = d->plan;
    P.N = c->N;
    P.n = n;
    P.K = c->K;
    P.L = d->L;
    P.v = d->v;
    int gs = 1;
    while (gs < d->L) gs *= 2;
    P.gs = gs;
    P.fpw = 64 / gs;
    P.nops = (int)s.ops.size();
    P.max_r1 = s.max_r1;
    // scratch layout, in 64-lane dword rows
    int r = 0;
    const int N = c->N;
    for (int dd = 0; dd <= qpd::kMaxDepth; ++dd) P.So[dd] = P.Uo[dd] = 0;
    for (int dd = 1; dd <= n - 1; ++dd) {
        P.So[dd] = r;
        r += dom != qpd::DOM_LUT ? 2 * (N >> dd) : std::max(1, ((N >> dd) + 3) / 4);
    }
    for (int dd = 1; dd <= n; ++dd) {
        P.Uo[dd] = r;
        r += std::max(1, ((N >> dd) + 31) / 32);
    }
    P.Ro = r;
    r += std::max(1, (N + 31) / 32);
    P.Ho = P.Ko = P.Io = r;
    if (c->kind == QPD_FASTSCL_LUT && s.max_r1 > 0) {
        P.Ho = r;
        r += (s.max_r1 + 31) / 32;
        P.Ko = r;
        r += 2 * s.max_r1;
        P.Io = r;
        if (s.max_r1 > qpd::stl::kThreshold) r += s.max_r1;
    }
    P.rows_per_wave = r;
    P.f_step = c->f_step;
    P.g_step = c->g_step;
    d->scratch_bytes_per_wave = (int64_t)r * 64 * 4;
    int mw = c->max_waves > 0 ? c->max_waves : 256 * 8;
    const int64_t cap = (int64_t)2 << 30;  // <= 2 GiB of scratch
    mw = (int)std::max<int64_t>(1, std::min<int64_t>(mw, cap / d->scratch_bytes_per_wave));
    d->max_waves = mw;

    std::vector<int32_t> info;
    for (int i = 0; i < N; ++i)
        if (c->frozen_bits[i] == 0) info.push_back(i);

#define QPD_TRY(x)            \
    do {                      \
        int rc_ = (x);        \
        if (rc_) {            \
            delete d;         \
            return rc_;       \
        }                     \
    } while (0)
    QPD_TRY(upload(d->ops, s.ops.data(), s.ops.size(), d->hs));
    QPD_TRY(upload(d->info_pos, info.data(), info.size(), d->hs));
    {
        std::vector<uint32_t> mask((N + 31) / 32, 0u);
        for (int i : info) mask[i >> 5] |= 1u << (i & 31);
        QPD_TRY(upload(d->info_mask, mask.data(), mask.size(), d->hs));
    }
    if (dom == qpd::DOM_UNIFORM) {
        QPD_TRY(upload(d->r_f, c->r_f, (size_t)N - 1, d->hs));
        QPD_TRY(upload(d->r_g, c->r_g, (size_t)N - 1, d->hs));
    } else if (dom == qpd::DOM_LLOYD) {
        QPD_TRY(upload(d->q_bnd, c->q_bnd, (size_t)c->q_bnd_count, d->hs));
        QPD_TRY(upload(d->q_rec, c->q_rec, (size_t)c->q_rec_count, d->hs));
        QPD_TRY(upload(d->bnd_off, c->bnd_off, 2 * ((size_t)N - 1), d->hs));
        QPD_TRY(upload(d->bnd_len, c->bnd_len, 2 * ((size_t)N - 1), d->hs));
        QPD_TRY(upload(d->rec_off, c->rec_off, 2 * ((size_t)N - 1), d->hs));
        QPD_TRY(upload(d->rec_len, c->rec_len, 2 * ((size_t)N - 1), d->hs));
    }
    if (dom == qpd::DOM_LUT) {
        const size_t vv = (size_t)c->v * c->v;
        QPD_TRY(upload(d->lut_f, c->lut_f, (size_t)c->lut_f_count * vv, d->hs));
        QPD_TRY(upload(d->lut_g, c->lut_g, (size_t)c->lut_g_count * 2 * vv, d->hs));
        QPD_TRY(upload(d->f_base, c->f_base, (size_t)N - 1, d->hs));
        QPD_TRY(upload(d->g_base, c->g_base, (size_t)N - 1, d->hs));
        QPD_TRY(upload(d->vcl, c->vcl, (size_t)c->vcl_rows * N * c->v, d->hs));
    }
    {
        hipError_t e = hipSuccess;
        if (d->engine == QPD_ENGINE_GENERIC) e = hipMalloc(&d->scratch.p, (size_t)d->scratch_bytes_per_wave * mw);
        if (e != hipSuccess) {
            delete d;
            return fail(QPD_E_DEVICE, std::string("scratch hipMalloc: ") + hipGetErrorString(e));
        }
        e = hipMalloc(&d->err.p, sizeof(int32_t));
        if (e == hipSuccess) e = hipMemsetAsync(d->err.p, 0, sizeof(int32_t), d->hs);
        if (e == hipSuccess) e = hipStreamSynchronize(d->hs);
        if (e != hipSuccess) {
            delete d;
            return fail(QPD_E_DEVICE, std::string("err hipMalloc: ") + hipGetErrorString(e));
        }
    }
    if (d->engine == QPD_ENGINE_FAST) QPD_TRY(build_fast(d, c, s));
#undef QPD_TRY
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
        if (rc) {
            delete d;
            return rc;
        }
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
    P.pm_init = (dom == qpd::DOM_LUT || c->kind == QPD_FASTSCL_LUT) ? __builtin_huge_val() : 1e300;
    P.out_k = d->out_bits;
    P.ca_A = d->ca_A;
    P.crc_n = d->crc_n;
    // bits compared after the A info bits: K - A (LUT kinds), crc_n (CASCLDecoder)
    P.ca_chk = cfg->kind == QPD_CASCL_FLOAT ? d->crc_n : d->K - d->ca_A;
    P.crc_q = d->crc_q;
    P.info_mask = (const uint32_t *)d->info_mask.p;
    d->fplan.out_k = d->out_bits;
    d->fplan.ca_A = d->ca_A;
    d->fplan.crc_n = d->crc_n;
    d->fplan.crc_q = d->crc_q;
    d->fplan.info_mask = (const uint32_t *)d->info_mask.p;
    {
        const int rc = build_host(d, cfg);
        if (rc) {
            delete d;
            return rc;
        }
    }
    *out = d;
    return QPD_OK;
}

void qpd_destroy(qpd_decoder *d) {
    if (!d) return;
    if (d->device >= 0) (void)hipSetDevice(d->device);
    delete d;  // ~qpd_decoder waits for the decoder's last work before any buffer is freed
}

int qpd_get_info(const qpd_decoder *d, qpd_info *info) {
    if (!d || !info) return fail(QPD_E_INVALID, "null argument");
    info->kind = d->pub_kind;
    info->out_bits = d->out_bits;
    info->host_max_frames = !d->hplan ? 0 : d->host_mode == QPD_HOST_GPU ? 0
                            : d->host_mode == QPD_HOST_CPU ? INT64_MAX : d->host_max_frames;
    info->N = d->N;
    info->K = d->K;
    info->L = d->L;
    info->v = d->v;
    info->num_ops = d->engine == QPD_ENGINE_FAST ? d->num_mops : (int32_t)d->ops_host.size();
    info->frames_per_wave = d->engine == QPD_ENGINE_FAST ? d->plan.fpw * d->sets : d->plan.fpw;
    info->lanes_per_frame = d->plan.gs;
    info->max_waves = d->max_waves;
    info->scratch_bytes_per_wave = d->scratch_bytes_per_wave;
    info->engine = d->engine;
    info->lds_bytes_per_wave = d->lds_bytes;
    info->lds_from_depth = d->engine == QPD_ENGINE_FAST ? d->fplan.lds_from : -1;
    info->prefix_ops = d->engine == QPD_ENGINE_FAST ? d->prefix_ops() : 0;
    info->last_engine = d->last_engine;
    // f / g ops of a node at depth d look up N >> (d + 1) symbols each; a leaf
    // pair's two decisions one each (SCLLUTDecoder.cpp:83-89, :157-164)
    int64_t lk = 0;
    for (const Op &o : d->ops_host)
        if (o.type == qpd::OP_F || o.type == qpd::OP_G) lk += d->N >> (o.d + 1);
        else if (o.type == qpd::OP_LEAF_L || o.type == qpd::OP_LEAF_R) lk += 1;
    info->lookups_per_path = lk;
    info->fast_variant = d->engine == QPD_ENGINE_FAST ? (d->pw1 ? 1 : 0) | (d->r1l ? 2 : 0) : 0;
    info->u8_staged = d->u8_staged;
    return QPD_OK;
}

}  // extern "C"

namespace {

// Launches of one device-buffer decode on stream st (caller: lock held,
// stream ordered).
// One fast-engine decode launch over Bc frames whose rows start at `in`
// (channel symbols, in_shift = n; or pre-pass rows, in_shift = n - 2).
int fast_launch(qpd_decoder *d, qpd::FastPlan fp, const int32_t *in, int64_t Bc, uint8_t *out, hipStream_t st,
                bool prefix = false) {
    const int sets = prefix ? d->pfx_sets : d->sets;
    const int64_t tw = (int64_t)fp.fpw * sets;  // frames per wave task
    const void *kfn = prefix ? prefix_kernel(d->kind, sets, d->pw1) : fast_kernel(d->kind, d->sets, d->l8, d->r1l, d->pw1, d->w16);
    if (!kfn) return fail(QPD_E_INVALID, "bad kind");
    const int64_t fgroups = (Bc + tw - 1) / tw;
    int fgrid = (int)std::min<int64_t>(fgroups, d->max_waves);
    if (!QPD_DYN) {
        // even out the rounds of the grid-stride loop (no partial last round)
        const int64_t rounds = (fgroups + fgrid - 1) / fgrid;
        fgrid = (int)((fgroups + rounds - 1) / rounds);
    }
    const qpd::MOp *ops_arg = fp.ops;
    fp.task_base = d->task_base;
    void *args[] = {&fp, &in, &Bc, &out, &ops_arg};
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

// pre-pass rows for `chunk` frames (N bytes each), grown on demand; on an
// allocation failure the chunk halves (fewer frames per decode launch, same
// results).  Returns the frames the buffer holds.
int64_t ensure_pre_rows(qpd_decoder *d, int64_t chunk, int *rc) {
    *rc = QPD_OK;
    // after a fallback the smaller buffer is the chunk: no device-wide hipFree
    // and failing hipMallocs on every later call
    if (d->pre_fell_back) chunk = std::min<int64_t>(chunk, d->pre_cap);
    if (d->pre_cap >= chunk) return std::min<int64_t>(chunk, d->pre_cap);
    if (d->pre_buf.p) (void)hipFree(d->pre_buf.p);
    d->pre_buf.p = nullptr;
    d->pre_cap = 0;
    const int64_t want = chunk;
    hipError_t e = hipErrorOutOfMemory;
    while (chunk >= 1 && (e = hipMalloc(&d->pre_buf.p, (size_t)chunk * (size_t)d->N)) != hipSuccess) {
        (void)hipGetLastError();
        d->pre_buf.p = nullptr;
        chunk /= 2;
    }
    if (e != hipSuccess) {
        *rc = fail(QPD_E_DEVICE, std::string("pre-pass rows hipMalloc: ") + hipGetErrorString(e));
        return 0;
    }
    d->pre_fell_back = d->pre_fell_back || e != hipSuccess || chunk < want;
    d->pre_cap = chunk;
    return chunk;
}

// Launches of one device-buffer decode on stream st (caller: lock held,
// stream ordered).
// Pre-mode: the root pre-pass on the channel symbols (int32, or uint8 read as
// they are), then the decode on its rows, chunk by chunk.  fp.in_vec: the
// symbol rows allow the reader's vector loads (chan_word8).
template <class In>
int decode_pre_mode(qpd_decoder *d, qpd::FastPlan fp, const In *d_symbols, int64_t B, uint8_t *d_out, hipStream_t st) {
    int rc = QPD_OK;
    const int64_t chunk = ensure_pre_rows(d, std::min<int64_t>(B, d->pre_chunk), &rc);
    if (rc) return rc;
    uint32_t *pre = (uint32_t *)d->pre_buf.p;
    for (int64_t f0 = 0; f0 < B; f0 += chunk) {
        int64_t Bc = std::min<int64_t>(chunk, B - f0);
        const In *sym = d_symbols + f0 * fp.N;
        fp.in_shift = fp.n;
        const int pgrid = (int)std::min<int64_t>(((Bc << (fp.n - 4)) + 255) / 256, 8192);
        void *pargs[] = {&fp, &sym, &Bc, &pre};
        rc = timed_launch(d, QPD_KC_PRE, st, [&]() -> int {
            QPD_HIP(hipLaunchKernel(reinterpret_cast<const void *>(&qpd::root_pre_kernel<In>), dim3(pgrid), dim3(256),
                                    pargs, 0, st));
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

// int32 staging for `chunk` frames of uint8 input, sized and grown as
// qpd_mc_decode sizes mc_sym: halved on an allocation failure, the smaller
// buffer kept from then on.  Returns the frames per chunk.
int64_t ensure_u8_stage(qpd_decoder *d, int64_t chunk, int *rc) {
    *rc = QPD_OK;
    if (d->u8_fell_back) chunk = std::min(chunk, d->u8_cap);
    if (d->u8_cap >= chunk) return chunk;
    if (d->u8_sym.p) (void)hipFree(d->u8_sym.p);
    d->u8_sym.p = nullptr;
    d->u8_cap = 0;
    hipError_t e = hipErrorOutOfMemory;
    const int64_t want = chunk;
    while (chunk >= 1 && (e = hipMalloc(&d->u8_sym.p, (size_t)chunk * d->N * sizeof(int32_t))) != hipSuccess) {
        (void)hipGetLastError();
        d->u8_sym.p = nullptr;
        chunk /= 2;
    }
    if (e != hipSuccess) {
        *rc = fail(QPD_E_DEVICE, std::string("uint8 staging hipMalloc: ") + hipGetErrorString(e));
        return 0;
    }
    d->u8_fell_back = chunk < want;
    d->u8_cap = chunk;
    return chunk;
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
    // <= 1 GB of int32 symbols per chunk (2^18 frames at N = 1024)
    const int64_t lim = d->u8_chunk ? d->u8_chunk : std::max<int64_t>(1, ((int64_t)1 << 30) / ((int64_t)d->N * 4));
    const int64_t chunk = ensure_u8_stage(d, std::min<int64_t>(B, lim), &rc);
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

int decode_f64_impl(qpd_decoder *d, const double *d_llr, int64_t B, uint8_t *d_out, hipStream_t st) {
    d->last_engine = QPD_RAN_GPU;
    d->u8_staged = 0;
    const int64_t groups = (B + d->plan.fpw - 1) / d->plan.fpw;
    const int grid = (int)std::min<int64_t>(groups, d->max_waves);
    return launch_generic(d, d_llr, B, d_out, grid, st);
}

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

// The Monte-Carlo generator on stream st: int32 symbols to `rows`, or (pre)
// the decoder's root pre-pass rows.  Caller: lock held, stream ordered.
int mc_launch(qpd_decoder *d, const qpd_mc_channel *ch, uint64_t seed, int64_t frame0, int64_t B, uint8_t *d_msg,
              int32_t *rows, bool pre, hipStream_t st) {
    if (!d->mc_pref.p) {  // per-decoder constants of the generator, built at the first call
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
        int rc2 = upload(d->mc_pref, pref.data(), pref.size(), d->hs);
        if (rc2) return rc2;
        rc2 = upload(d->mc_crc, tab.data(), tab.size(), d->hs);
        if (rc2) return rc2;
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
    int dev = 0, ncu = 256, per_cu = 0;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
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

// One call's work on stream st, ordered after the decoder's previous work on
// any other stream, under the handle's lock.
template <class F>
int ordered(qpd_decoder *d, hipStream_t st, F &&work) {
    std::lock_guard<std::mutex> lk(d->mu);
    int rc = set_device(d);
    if (rc) return rc;
    if ((rc = order_on(d, st))) return rc;
    rc = work();
    const int mrc = mark_on(d, st);  // also after a failed launch: earlier launches of the call may be queued
    return rc ? rc : mrc;
}

}  // namespace

extern "C" {

int qpd_decode(qpd_decoder *d, const int32_t *d_symbols, int64_t B, uint8_t *d_out, void *stream) {
    if (!d) return fail(QPD_E_INVALID, "null decoder");
    if (d->dom != qpd::DOM_LUT) return fail(QPD_E_INVALID, "this decoder takes float64 LLRs: use qpd_decode_f64");
    if (B < 0) return fail(QPD_E_INVALID, "negative batch");
    if (B == 0) return QPD_OK;
    if (!d_symbols || !d_out) return fail(QPD_E_INVALID, "null buffer");
    hipStream_t st = (hipStream_t)stream;
    return ordered(d, st, [&]() { return decode_impl(d, d_symbols, B, d_out, st); });
}

int qpd_decode_u8(qpd_decoder *d, const uint8_t *d_symbols, int64_t B, uint8_t *d_out, void *stream) {
    if (!d) return fail(QPD_E_INVALID, "null decoder");
    if (d->dom != qpd::DOM_LUT) return fail(QPD_E_INVALID, "this decoder takes float64 LLRs: use qpd_decode_f64");
    if (B < 0) return fail(QPD_E_INVALID, "negative batch");
    if (B == 0) return QPD_OK;
    if (!d_symbols || !d_out) return fail(QPD_E_INVALID, "null buffer");
    hipStream_t st = (hipStream_t)stream;
    return ordered(d, st, [&]() { return decode_u8_impl(d, d_symbols, B, d_out, st); });
}

int qpd_decode_f64(qpd_decoder *d, const double *d_llr, int64_t B, uint8_t *d_out, void *stream) {
    if (!d) return fail(QPD_E_INVALID, "null decoder");
    if (d->dom == qpd::DOM_LUT) return fail(QPD_E_INVALID, "LUT decoders take int32 channel symbols: use qpd_decode");
    if (B < 0) return fail(QPD_E_INVALID, "negative batch");
    if (B == 0) return QPD_OK;
    if (!d_llr || !d_out) return fail(QPD_E_INVALID, "null buffer");
    hipStream_t st = (hipStream_t)stream;
    return ordered(d, st, [&]() { return decode_f64_impl(d, d_llr, B, d_out, st); });
}

}  // extern "C"

static int input_error(int32_t flag) {
    std::string msg;
    if (flag & qpd::ERR_SYMBOL) msg += "channel symbol outside [0, v) in decoder input; ";
    if (flag & qpd::ERR_LLOYD) msg += "Lloyd bisect index outside the reconstruction list (reference UB); ";
    if (flag & qpd::ERR_NAN_PM) msg += "NaN path metric reached the list sort (reference UB); ";
    msg.resize(msg.size() - 2);
    return fail(QPD_E_INPUT, msg);
}

static int ensure(DeviceBuf &b, size_t &have, size_t need) {
    if (have >= need) return QPD_OK;
    if (b.p) {
        QPD_HIP(hipFree(b.p));
        b.p = nullptr;
    }
    QPD_HIP(hipMalloc(&b.p, need));
    have = need;
    return QPD_OK;
}

// One synchronous host-buffer decode: input staged through pinned memory,
// H2D copy, decode and D2H copies of the bits and the error word queued on
// the handle's own stream, one stream synchronization.  (What a per-frame
// decode(symbols) call of the reference drivers costs here: tools/latency.py.)
// Whether a host-buffer call of B frames runs on the host engine.
static bool host_engine_takes(const qpd_decoder *d, int64_t B) {
    if (!d->hplan || d->host_mode == QPD_HOST_GPU) return false;
    return d->host_mode == QPD_HOST_CPU || B <= d->host_max_frames;
}

// B frames on the host engine, one after another, under the handle's lock.
// The GPU work of the decoder is not touched (the engine has its own state),
// so no stream ordering is needed.
template <class Eng, class In>
static int host_engine_run(qpd_decoder *d, Eng *eng, const In *h_in, int64_t B, uint8_t *h_out) {
    std::lock_guard<std::mutex> lk(d->mu);
    d->last_engine = QPD_RAN_HOST;
    d->u8_staged = 0;
    int32_t flag = 0;
    for (int64_t b = 0; b < B; ++b) flag |= eng->decode(h_in + b * d->N, h_out + b * d->out_bits);
    return flag ? input_error(flag) : QPD_OK;
}

template <class In, class Dec>
static int host_roundtrip(qpd_decoder *d, const In *h_in, int64_t B, uint8_t *h_out, Dec dec) {
    const size_t in_b = (size_t)B * d->N * sizeof(In), out_b = (size_t)B * d->out_bits;
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
        std::memcpy(h_out, pin + out_at, out_b);
        int32_t flag = 0;
        std::memcpy(&flag, pin + err_at, sizeof(flag));
        if (flag) {
            QPD_HIP(hipMemsetAsync(d->err.p, 0, sizeof(int32_t), hs));
            QPD_HIP(hipStreamSynchronize(hs));
            return input_error(flag);
        }
        return QPD_OK;
    });
}

extern "C" {

int qpd_check_input_error(qpd_decoder *d) {
    if (!d) return fail(QPD_E_INVALID, "null decoder");
    hipStream_t hs = d->hs;
    return ordered(d, hs, [&]() -> int {
        // hs waits for the decoder's last launch (any stream); the flag is
        // read and cleared on hs, which later calls on other streams wait for
        int32_t flag = 0;
        QPD_HIP(hipMemcpyAsync(&flag, d->err.p, sizeof(flag), hipMemcpyDeviceToHost, hs));
        QPD_HIP(hipStreamSynchronize(hs));
        if (flag) {
            QPD_HIP(hipMemsetAsync(d->err.p, 0, sizeof(int32_t), hs));
            QPD_HIP(hipStreamSynchronize(hs));
            return input_error(flag);
        }
        return QPD_OK;
    });
}

int qpd_decode_host(qpd_decoder *d, const int32_t *h_symbols, int64_t B, uint8_t *h_out) {
    if (!d) return fail(QPD_E_INVALID, "null decoder");
    if (d->dom != qpd::DOM_LUT) return fail(QPD_E_INVALID, "this decoder takes float64 LLRs: use qpd_decode_f64_host");
    if (B <= 0) return B == 0 ? QPD_OK : fail(QPD_E_INVALID, "negative batch");
    if (!h_symbols || !h_out) return fail(QPD_E_INVALID, "null buffer");
    if (host_engine_takes(d, B)) return host_engine_run(d, d->heng_lut.get(), h_symbols, B, h_out);
    return host_roundtrip(d, h_symbols, B, h_out,
                          [&](const int32_t *in, uint8_t *out, hipStream_t st) { return decode_impl(d, in, B, out, st); });
}

int qpd_decode_u8_host(qpd_decoder *d, const uint8_t *h_symbols, int64_t B, uint8_t *h_out) {
    if (!d) return fail(QPD_E_INVALID, "null decoder");
    if (d->dom != qpd::DOM_LUT) return fail(QPD_E_INVALID, "this decoder takes float64 LLRs: use qpd_decode_f64_host");
    if (B <= 0) return B == 0 ? QPD_OK : fail(QPD_E_INVALID, "negative batch");
    if (!h_symbols || !h_out) return fail(QPD_E_INVALID, "null buffer");
    if (host_engine_takes(d, B)) return host_engine_run(d, d->heng_lut.get(), h_symbols, B, h_out);
    return host_roundtrip(d, h_symbols, B, h_out,
                          [&](const uint8_t *in, uint8_t *out, hipStream_t st) { return decode_u8_impl(d, in, B, out, st); });
}

int qpd_decode_f64_host(qpd_decoder *d, const double *h_llr, int64_t B, uint8_t *h_out) {
    if (!d) return fail(QPD_E_INVALID, "null decoder");
    if (d->dom == qpd::DOM_LUT) return fail(QPD_E_INVALID, "LUT decoders take int32 channel symbols: use qpd_decode_host");
    if (B <= 0) return B == 0 ? QPD_OK : fail(QPD_E_INVALID, "negative batch");
    if (!h_llr || !h_out) return fail(QPD_E_INVALID, "null buffer");
    if (host_engine_takes(d, B)) return host_engine_run(d, d->heng_f64.get(), h_llr, B, h_out);
    return host_roundtrip(d, h_llr, B, h_out,
                          [&](const double *in, uint8_t *out, hipStream_t st) { return decode_f64_impl(d, in, B, out, st); });
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
    if (!d || !ch) return fail(QPD_E_INVALID, "null argument");
    if (B < 0 || frame0 < 0) return fail(QPD_E_INVALID, "negative frame range");
    if (B == 0) return QPD_OK;
    if (!d_msg || !d_symbols) return fail(QPD_E_INVALID, "null buffer");
    int rc = check_channel(ch);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    return ordered(d, st, [&]() { return mc_launch(d, ch, seed, frame0, B, d_msg, d_symbols, false, st); });
}

int qpd_mc_decode(qpd_decoder *d, const qpd_mc_channel *ch, uint64_t seed, int64_t frame0, int64_t B, uint8_t *d_msg,
                  uint8_t *d_out, int64_t *d_counts, void *stream) {
    if (!d || !ch) return fail(QPD_E_INVALID, "null argument");
    if (d->dom != qpd::DOM_LUT) return fail(QPD_E_INVALID, "qpd_mc_decode needs a LUT decoder (int32 channel symbols)");
    if (B < 0 || frame0 < 0) return fail(QPD_E_INVALID, "negative frame range");
    if (B == 0) return QPD_OK;
    if (!d_msg || !d_out) return fail(QPD_E_INVALID, "null buffer");
    int rc = check_channel(ch);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    return ordered(d, st, [&]() -> int {
        // fused: the generator writes the root pre-pass rows the decode
        // kernel reads (fast engine in pre-mode; symbols < q <= v need no
        // range check); else int32 symbols in a buffer of its own
        const bool fused = d->engine == QPD_ENGINE_FAST && d->pre && ch->q <= d->v;
        d->last_engine = QPD_RAN_GPU;
        d->u8_staged = 0;
        int64_t chunk;
        if (fused) {
            int r0 = QPD_OK;
            chunk = ensure_pre_rows(d, std::min<int64_t>(B, d->pre_chunk), &r0);
            if (r0) return r0;
        } else {
            // int32 symbols of <= 1 GB per chunk (2^18 frames at N = 1024); halved
            // on an allocation failure, and the smaller buffer kept from then on
            chunk = std::min<int64_t>(B, std::max<int64_t>(1, ((int64_t)1 << 30) / ((int64_t)d->N * 4)));
            if (d->mc_sym_fell_back) chunk = std::min(chunk, d->mc_sym_cap);
            if (d->mc_sym_cap < chunk) {
                if (d->mc_sym.p) QPD_HIP(hipFree(d->mc_sym.p));
                d->mc_sym.p = nullptr;
                d->mc_sym_cap = 0;
                hipError_t e = hipErrorOutOfMemory;
                const int64_t want = chunk;
                while (chunk >= 1 && (e = hipMalloc(&d->mc_sym.p, (size_t)chunk * d->N * sizeof(int32_t))) != hipSuccess) {
                    (void)hipGetLastError();
                    d->mc_sym.p = nullptr;
                    chunk /= 2;
                }
                if (e != hipSuccess) return fail(QPD_E_DEVICE, std::string("Monte-Carlo symbols hipMalloc: ") + hipGetErrorString(e));
                d->mc_sym_fell_back = chunk < want;
                d->mc_sym_cap = chunk;
            }
            chunk = std::min(chunk, d->mc_sym_cap);
        }
        DeviceBuf &buf = fused ? d->pre_buf : d->mc_sym;
        for (int64_t f0 = 0; f0 < B; f0 += chunk) {
            const int64_t Bc = std::min<int64_t>(chunk, B - f0);
            int r = mc_launch(d, ch, seed, frame0 + f0, Bc, d_msg + f0 * d->out_bits, (int32_t *)buf.p, fused, st);
            if (r) return r;
            uint8_t *out = d_out + f0 * d->out_bits;
            r = fused ? decode_pre_rows(d, (const uint32_t *)buf.p, Bc, out, st)
                      : decode_impl(d, (const int32_t *)buf.p, Bc, out, st);
            if (r) return r;
        }
        if (d_counts) {  // the driver's error counters over the whole range
            int dev = 0, ncu = 256;
            (void)hipGetDevice(&dev);
            (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
            const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((B + 3) / 4, (int64_t)ncu * 8));
            hipLaunchKernelGGL(qpd::mc_count_kernel, dim3(grid), dim3(256), 0, st, d_out, d_msg, B, d->out_bits,
                               (unsigned long long *)d_counts);
            QPD_HIP(hipGetLastError());
        }
        return QPD_OK;
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

