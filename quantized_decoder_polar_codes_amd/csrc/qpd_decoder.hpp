// qpd_decoder.hpp -- the decoder handle of the C-ABI (struct qpd_decoder) and
// what every entry point shares: the error string, device buffers, uploads,
// the ordering of one decoder's work across streams and host threads, and
// launches bracketed by profiling events.  Host code.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "qpd.h"
#include "qpd_generic.hip"
#include "qpd_fast_plan.hpp"
#include "qpd_chunk.hpp"
#include "qpd_host.hpp"
#include "qpd_status.hpp"
#include "qpd_list.hpp"
#include "qpd_search.hpp"
#include "qpd_tx.hpp"

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

struct DeviceBuf {
    void *p = nullptr;
    ~DeviceBuf() {
        if (p) (void)hipFree(p);
    }
};

// A chunk buffer (qpd_chunk.hpp) in device memory, freed with the decoder.
struct DeviceChunk : qpd::ChunkBuf {
    ~DeviceChunk() {
        if (p) (void)hipFree(p);
    }
    // The frames per chunk; 0 with *rc = QPD_E_DEVICE (`what`, then the last
    // hipMalloc's error) when not even one frame could be allocated.
    int64_t reserve(int64_t want, size_t bytes_per_frame, const char *what, int *rc) {
        hipError_t e = hipErrorOutOfMemory;
        const int64_t got = ChunkBuf::reserve(
            want, bytes_per_frame,
            [&e](size_t bytes) -> void * {
                void *q = nullptr;
                if ((e = hipMalloc(&q, bytes)) == hipSuccess) return q;
                (void)hipGetLastError();
                return nullptr;
            },
            [](void *q) { (void)hipFree(q); });
        *rc = got ? QPD_OK : fail(QPD_E_DEVICE, std::string(what) + hipGetErrorString(e));
        return got;
    }
};

// CUs of the current device (256 where the query fails).
int device_cus() {
    int dev = 0, ncu = 256;
    (void)hipGetDevice(&dev);
    (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
    return ncu;
}

}  // namespace

struct qpd_decoder {
    int kind, N, n, K, L, v, device;  // kind: the kernel family (SC/SCL/FastSC/FastSCL LUT ids)
    int dom = 0;                      // qpd::Dom symbol domain
    int max_waves;
    int64_t scratch_bytes_per_wave;
    int engine = QPD_ENGINE_GENERIC;
    int lds_bytes = 0;
    int lds_tab_bytes = 0;  // of lds_bytes: the f / g ops' byte tables (SCL-LUT), the first bytes of the dynamic LDS
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
    bool row_lo = false;      // ... whose rows are in lookup order (FastHostPlan::row_lo)
    int64_t pre_chunk = 0;    // frames per pre-pass chunk
    DeviceChunk pre_rows;     // pre-pass rows of one chunk (N bytes per frame)
    DeviceChunk mc_sym;       // qpd_mc_decode without a fused pre-pass: int32 symbols of one chunk
    DeviceChunk mc_llr;       // qpd_mc_decode_f64: float64 LLRs of one chunk (qpd_chunk.hpp: mc_llr_chunk_frames)
    DeviceBuf mc_rec;         // qpd_mc_llr / qpd_mc_decode_f64 with rec: the reconstruction table's device copy
    std::vector<double> mc_rec_host;  // what mc_rec holds (empty: nothing)
    std::unique_ptr<qpd_tx::Code> tx_code;  // qpd_encode_host: the encoder's constants (built at the first call)
    DeviceChunk u8_sym;       // qpd_decode_u8 / qpd_decode_llr outside pre-mode: int32 symbols of one chunk
    int64_t u8_chunk = 0;    // QPD_U8_CHUNK (tests): frames per staging chunk (0: 1 GB of int32 symbols)
    int u8_staged = 0;       // qpd_info.u8_staged: the last decode call widened its input into u8_sym
    bool llr_coop = true;    // qpd_decode_llr in pre-mode: the front kernel's cooperative read (QPD_LLR_COOP=0: per owner)
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
    DeviceBuf h_in, h_out, h_st;  // h_st: qpd_decode_status_host's metrics, then its flags
    size_t h_in_bytes = 0, h_out_bytes = 0, h_st_bytes = 0;
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
    // qpd_decode_status, for the length of the call (under `mu`): what its launches
    // write besides the bits, and the call's d_out -- a chunk's launch finds its
    // first frame from its own `out` (status_at, qpd_capi_decode.hpp).
    qpd_stat::Req st_req;
    const uint8_t *st_out0 = nullptr;
    // qpd_decode_list, likewise (st_out0: the call's d_out, or ls_out when it gave none)
    qpd_list::Req ls_req;
    DeviceBuf ls_out;  // the bits of a qpd_decode_list call without d_out
    size_t ls_out_bytes = 0;
    DeviceBuf h_ls;  // qpd_decode_list_host's device outputs: bits, metrics, flags, chosen
    size_t h_ls_bytes = 0;
    // qpd_decode_search, likewise; the mask set's words in a device buffer of the handle
    // (QPD_MAX_SEARCH_MASKS words), uploaded on the handle's own stream when it changes
    // (SearchScope, qpd_capi_decode.hpp); sr_set_host: what is resident
    qpd_search::Req sr_req;
    DeviceBuf sr_set;
    std::vector<uint32_t> sr_set_host;
    DeviceBuf h_sr;  // qpd_decode_search_host's device outputs
    size_t h_sr_bytes = 0;
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

}  // namespace
