// Test harness (CPU): qpd_create's host-only decisions (csrc/qpd_config.hpp)
// built with g++ beside the tests, one C function per decision for ctypes
// (tests/test_capi_host.py).
#include <cstdio>

#include "qpd_config.hpp"

namespace {

void put(const std::string &err, char *msg, int msg_len) {
    if (msg && msg_len > 0) snprintf(msg, (size_t)msg_len, "%s", err.c_str());
}

}  // namespace

extern "C" {

// validate's return code; the message in msg; out3 = {n, family, domain} where it accepts.
int ch_validate(const qpd_config *c, char *msg, int msg_len, int *out3) {
    std::string err;
    int n = -1, fam = -1, dom = -1;
    const int rc = qpd_cfg::validate(c, &n, &fam, &dom, err);
    put(err, msg, msg_len);
    out3[0] = n, out3[1] = fam, out3[2] = dom;
    return rc;
}

int ch_engine(int dom, int f_step, int g_step, int v, int kind, int L, int want, char *msg, int msg_len) {
    std::string err;
    const int e = qpd_cfg::choose_engine(dom, f_step, g_step, v, kind, L, want, err);
    put(err, msg, msg_len);
    return e;
}

// So[0..16], Uo[0..16], Ro, Ho, Ko, Io, rows_per_wave: 39 values.
void ch_layout(int kind, int dom, int N, int n, int max_r1, int32_t *out39) {
    const qpd_cfg::GenericLayout G = qpd_cfg::generic_layout(kind, dom, N, n, max_r1);
    int k = 0;
    for (int d = 0; d <= qpd::kMaxDepth; ++d) out39[k++] = G.So[d];
    for (int d = 0; d <= qpd::kMaxDepth; ++d) out39[k++] = G.Uo[d];
    out39[k++] = G.Ro, out39[k++] = G.Ho, out39[k++] = G.Ko, out39[k++] = G.Io, out39[k++] = G.rows_per_wave;
}

uint32_t ch_crc_taps(int crc_n, const int32_t *loc, int count) { return qpd_cfg::crc_taps(crc_n, loc, count); }

int64_t ch_host_max_frames(int N, int n, int L) { return qpd_cfg::host_max_frames(N, n, L); }

int ch_ilog2_exact(int N) { return qpd_cfg::ilog2_exact(N); }

}  // extern "C"
