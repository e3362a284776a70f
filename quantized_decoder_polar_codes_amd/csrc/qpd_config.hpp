// qpd_config.hpp -- what qpd_create decides from a qpd_config before anything
// touches the device: the refusals, the engine, the generic engine's scratch
// rows, the CRC tap word, the host engine's crossover.  Host code without HIP
// (g++ builds it beside qpd_schedule.hpp; tests/test_capi_host.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "qpd.h"
#include "qpd_schedule.hpp"
#include "qpd_types.hpp"
#include "stl_sort.hpp"

namespace qpd_cfg {

using qpd_sched::family_of;
using qpd_sched::is_ca;
using qpd_sched::special_of;

inline int ilog2_exact(int N) {
    int n = 0;
    while ((1 << n) < N) ++n;
    return ((1 << n) == N) ? n : -1;
}

inline int refuse(std::string &err, int code, const char *msg) {
    err = msg;
    return code;
}

// QPD_OK with log2(N), the kernel family and the symbol domain of the kind
// (family_of), or the refusal with its message in `err`.
inline int validate(const qpd_config *c, int *n_out, int *fam_out, int *dom_out, std::string &err) {
    if (!c) return refuse(err, QPD_E_INVALID, "null config");
    int fam = 0, dom = 0;
    if (!family_of(c->kind, &fam, &dom)) return refuse(err, QPD_E_INVALID, "unknown decoder kind");
    if (is_ca(c->kind)) {
        if (c->crc_n < 1 || c->crc_n > 32) return refuse(err, QPD_E_INVALID, "crc_n must be in [1, 32]");
        if (c->kind == QPD_CASCL_FLOAT) {
            // CASCLDecoder.cpp:218-226 compares crc_n bits after the A info bits:
            // A + crc_n > K would read past the decoded info bits (UB there).
            if (c->A < 1 || c->A + c->crc_n > c->K) return refuse(err, QPD_E_INVALID, "CASCLDecoder needs 1 <= A and A + crc_n <= K");
        } else if (c->A < 1 || c->A > c->K || c->K - c->A > c->crc_n) {
            // CRC-aided LUT output (CASCLLUTDecoder.cpp:263-302): K - A > crc_n would
            // read past the reference's check code (UB there), so it is rejected here.
            return refuse(err, QPD_E_INVALID, "CRC-aided kinds need 1 <= A <= K and K - A <= crc_n");
        }
        if (c->crc_loc_count < 0 || (c->crc_loc_count > 0 && !c->crc_loc)) return refuse(err, QPD_E_INVALID, "bad crc_loc");
        for (int i = 0; i < c->crc_loc_count; ++i)
            if (c->crc_loc[i] < 0 || c->crc_loc[i] > c->crc_n) return refuse(err, QPD_E_INVALID, "crc_loc entry outside [0, crc_n]");
    }
    const int n = ilog2_exact(c->N);
    if (c->N < 2 || n < 0 || n > qpd::kMaxDepth) return refuse(err, QPD_E_INVALID, "N must be a power of two in [2, 65536]");
    if (!c->frozen_bits) return refuse(err, QPD_E_INVALID, "frozen_bits is NULL");
    int zeros = 0;
    for (int i = 0; i < c->N; ++i) {
        if (c->frozen_bits[i] != 0 && c->frozen_bits[i] != 1)
            return refuse(err, QPD_E_INVALID, "frozen_bits entries must be 0 or 1");
        zeros += c->frozen_bits[i] == 0;
    }
    if (zeros != c->K) return refuse(err, QPD_E_INVALID, "K must equal the number of information (0) entries of frozen_bits");
    *n_out = n;
    *fam_out = fam;
    *dom_out = dom;
    const bool list = fam == QPD_SCL_LUT || fam == QPD_FASTSCL_LUT;
    if (list && (c->L < 1 || c->L > qpd::kMaxLWide))
        return refuse(err, QPD_E_UNSUPPORTED, "list size L must be in [1, 32]");
    if (fam == QPD_FASTSC_LUT || fam == QPD_FASTSCL_LUT) {
        if (!c->node_type) return refuse(err, QPD_E_INVALID, "node_type is required for the Fast decoders");
        if (special_of(fam, c->node_type, 0) >= 0)
            return refuse(err, QPD_E_UNSUPPORTED, "root node labelled special (undefined behaviour in the reference)");
    }
    if (dom == qpd::DOM_UNIFORM && (!c->r_f || !c->r_g)) return refuse(err, QPD_E_INVALID, "uniform kinds need r_f and r_g");
    if (dom == qpd::DOM_LLOYD) {
        if (!c->q_bnd || !c->q_rec || !c->bnd_off || !c->bnd_len || !c->rec_off || !c->rec_len)
            return refuse(err, QPD_E_INVALID, "Lloyd kinds need boundary and reconstruction tables");
        for (int k = 0; k < 2 * (c->N - 1); ++k) {
            if (c->bnd_len[k] < 1 || c->bnd_off[k] < 0 || (long)c->bnd_off[k] + c->bnd_len[k] > c->q_bnd_count)
                return refuse(err, QPD_E_INVALID, "Lloyd boundary list outside q_bnd (or empty)");
            if (c->rec_len[k] < 1 || c->rec_off[k] < 0 || (long)c->rec_off[k] + c->rec_len[k] > c->q_rec_count)
                return refuse(err, QPD_E_INVALID, "Lloyd reconstruction list outside q_rec (or empty)");
        }
    }
    if (dom != qpd::DOM_LUT) return QPD_OK;
    if (c->v < 2 || c->v > 256) return refuse(err, QPD_E_INVALID, "alphabet size v must be in [2, 256]");
    if (!c->lut_f || !c->lut_g || !c->f_base || !c->g_base || !c->vcl) return refuse(err, QPD_E_INVALID, "null table pointer");
    if ((c->f_step != 0 && c->f_step != 1) || (c->g_step != 0 && c->g_step != 1))
        return refuse(err, QPD_E_INVALID, "f_step/g_step must be 0 or 1");
    if (c->vcl_rows < n) return refuse(err, QPD_E_INVALID, "vcl_rows must be >= log2(N)");
    const int vv = c->v * c->v;
    for (int p = 0; p < c->N - 1; ++p) {
        const int depth = 31 - __builtin_clz((unsigned)(p + 1));
        const int last = (c->N >> (depth + 1)) - 1;
        const long fl = (long)c->f_base[p] + (long)last * c->f_step;
        const long gl = (long)c->g_base[p] + (long)last * c->g_step;
        if (c->f_base[p] < 0 || fl >= c->lut_f_count) return refuse(err, QPD_E_INVALID, "f_base/f_step index outside lut_f");
        if (c->g_base[p] < 0 || gl >= c->lut_g_count) return refuse(err, QPD_E_INVALID, "g_base/g_step index outside lut_g");
    }
    for (long i = 0; i < (long)c->lut_f_count * vv; ++i)
        if (c->lut_f[i] >= c->v) return refuse(err, QPD_E_INVALID, "lut_f entry outside [0, v)");
    for (long i = 0; i < (long)c->lut_g_count * 2 * vv; ++i)
        if (c->lut_g[i] >= c->v) return refuse(err, QPD_E_INVALID, "lut_g entry outside [0, v)");
    for (long i = 0; i < (long)n * c->N * c->v; ++i)
        if (!std::isfinite(c->vcl[i])) return refuse(err, QPD_E_INVALID, "vcl rows 0..n-1 must be finite");
    return QPD_OK;
}

// The engine of a decoder of family `kind` with list size L (1 for the SC
// families), asked for `want` (QPD_ENGINE_*; anything else counts as AUTO):
// QPD_ENGINE_FAST / _GENERIC, or QPD_E_UNSUPPORTED with its message in `err`.
// L > 8 (2L > 16: libstdc++ introsort, replayed where ties make it matter): up to L = 16 on
// the fast engine (lane groups of 16, select_survivors16) -- SCL-LUT under AUTO, FastSCL-LUT
// only on an explicit request (fast_avail): AUTO keeps it on the generic engine
inline int choose_engine(int dom, int f_step, int g_step, int v, int kind, int L, int want, std::string &err) {
    const bool fast_base = dom == qpd::DOM_LUT && f_step == 0 && g_step == 0 && v <= 16;
    const bool fast_auto = fast_base && (L <= qpd::kMaxL || (kind == QPD_SCL_LUT && L <= 2 * qpd::kMaxL));
    const bool fast_avail = fast_auto || (fast_base && kind == QPD_FASTSCL_LUT && L <= 2 * qpd::kMaxL);
    if (want == QPD_ENGINE_FAST && !fast_avail)
        return refuse(err, QPD_E_UNSUPPORTED,
                      "fast engine needs LUT symbols with one table per node (f_step = g_step = 0), v <= 16 and L <= 8 "
                      "(SCL-LUT and, on request, FastSCL-LUT: L <= 16)");
    return want == QPD_ENGINE_FAST ? QPD_ENGINE_FAST
           : (want == QPD_ENGINE_GENERIC || !fast_auto) ? QPD_ENGINE_GENERIC : QPD_ENGINE_FAST;
}

// The generic engine's scratch layout, in 64-lane dword rows (DevPlan's fields
// of the same names, qpd_generic.hip).
struct GenericLayout {
    int32_t So[qpd::kMaxDepth + 1], Uo[qpd::kMaxDepth + 1], Ro, Ho, Ko, Io;
    int32_t rows_per_wave;
};

inline GenericLayout generic_layout(int kind, int dom, int N, int n, int max_r1) {
    GenericLayout P;
    int r = 0;
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
    if (kind == QPD_FASTSCL_LUT && max_r1 > 0) {
        P.Ho = r;
        r += (max_r1 + 31) / 32;
        P.Ko = r;
        r += 2 * max_r1;
        P.Io = r;
        if (max_r1 > qpd::stl::kThreshold) r += max_r1;
    }
    P.rows_per_wave = r;
    return P;
}

// The CRC register's tap word from the generator's coefficient list.
inline uint32_t crc_taps(int crc_n, const int32_t *crc_loc, int crc_loc_count) {
    uint32_t q = 0;
    for (int i = 0; i < crc_loc_count; ++i) {
        const int j = crc_loc[i];  // coefficient j -> register bit crc_n - j (j = 0: leading, drops out)
        if (j >= 1) q |= 1u << (crc_n - j);
    }
    return q;
}

// The batch size up to which QPD_HOST_AUTO prefers the host engine
// (qpd_host.hpp) for a host-buffer call.  The crossover is a cost model fitted
// to the per-call latencies measured on MI355X (tools/latency.py,
// profiles/r02_latency.jsonl, re-checked on profiles/r03af_latency.jsonl).
// Per frame on the host engine ~ its lookups (N log2 N per path) plus, for
// lists, the forks (re-fitted to the round-3 engine, profiles/
// r03af_latency.jsonl: SC-LUT N=128 2.8 us, N=1024 15.5 us, SCL-LUT N=1024
// L=8 0.154 ms); a GPU call ~ 55 us of launches, copies and synchronization
// plus one wave running the serial schedule (SC-LUT N=128 0.11 ms, N=1024
// 0.91 ms, SCL-LUT N=1024 L=8 1.07 ms, same file) -- flat in the batch up to
// thousands of frames.
inline int64_t host_max_frames(int N, int n, int L) {
    const double nn = (double)N * n;
    const double host_us = 0.00136 * nn * L + (L > 1 ? 0.005 * L * N : 0.0) + 1.6;
    const double gpu_us = 55.0 + 0.083 * nn + (L > 1 ? 0.02 * nn : 0.0);
    return std::max<int64_t>(1, (int64_t)(gpu_us / host_us));
}

}  // namespace qpd_cfg
