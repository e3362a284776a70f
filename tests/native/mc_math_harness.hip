// Device harness of the Monte-Carlo generator's arithmetic (csrc/qpd_mc.hip): one small
// kernel that runs the generator's `noise` step -- mc_one_m, mc_log, sqrt, mc_sincos, the
// product's own functions, with the product's floating-point contraction setting -- on
// Philox words the caller chooses, and one that runs philox4x32_10 on chosen counters and
// keys.  tests/test_gpu_mc_math.py compares the results with mpmath and with the numpy
// restatement (tests/mc_ref.py).
#include "qpd_fast_lookup.hpp"  // lut_vec, which qpd_mc.hip's PRE mode calls
#include "qpd_mc.hip"

#ifndef QPD_MCM_BUILD_ID
#define QPD_MCM_BUILD_ID "unstamped"
#endif

namespace {

// What mc_frames_kernel's `noise` computes from the four words of one Philox draw.
__global__ __launch_bounds__(256) void noise_kernel(int64_t n, const uint32_t *__restrict__ a,
                                                    const uint32_t *__restrict__ b, const uint32_t *__restrict__ c,
                                                    const uint32_t *__restrict__ d, double *__restrict__ u1o,
                                                    double *__restrict__ u2o, double *__restrict__ lgo,
                                                    double *__restrict__ sno, double *__restrict__ cso,
                                                    double *__restrict__ nz0, double *__restrict__ nz1) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double u1 = 2.0 - qpd::mc_one_m(a[i], b[i]);  // (0, 1]
    const double u2 = qpd::mc_one_m(c[i], d[i]) - 1.0;  // [0, 1)
    const double lg = qpd::mc_log(u1);
    const double rad = sqrt(-2.0 * lg);
    double sn, cs;
    qpd::mc_sincos(6.283185307179586 * u2, &sn, &cs);
    u1o[i] = u1;
    u2o[i] = u2;
    lgo[i] = lg;
    sno[i] = sn;
    cso[i] = cs;
    nz0[i] = rad * cs;
    nz1[i] = rad * sn;
}

// One block per key (the generator's key is wave-uniform: philox4x32_10 keeps it in
// scalar registers), nc counters per key.  keys: [nk][2], ctr / out: [nk][nc][4].
__global__ __launch_bounds__(64) void philox_kernel(int nc, const uint32_t *__restrict__ keys,
                                                    const uint32_t *__restrict__ ctr, uint32_t *__restrict__ out) {
    const uint32_t k0 = __builtin_amdgcn_readfirstlane(keys[2 * blockIdx.x]);
    const uint32_t k1 = __builtin_amdgcn_readfirstlane(keys[2 * blockIdx.x + 1]);
    for (int j = threadIdx.x; j < nc; j += 64) {
        const size_t at = 4 * ((size_t)blockIdx.x * nc + j);
        const qpd::Philox4 r = qpd::philox4x32_10(ctr[at], ctr[at + 1], ctr[at + 2], ctr[at + 3], k0, k1);
        for (int w = 0; w < 4; ++w) out[at + w] = r.v[w];
    }
}

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

}  // namespace

extern "C" {

const char *qpd_mcm_build_id() {
    static const char tag[] = "qpd-mcm-build-id:" QPD_MCM_BUILD_ID;
    return tag + 17;
}

#define MCM_TRY(x) \
    if ((e = (x)) != hipSuccess) return (int)e

// out: [7][n] doubles -- u1, u2, mc_log(u1), sin, cos, nz0, nz1.  Returns the HIP error code, -1 for bad arguments.
int qpd_mcm_noise(int64_t n, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, double *out) {
    if (n < 1 || n > (1 << 24) || !a || !b || !c || !d || !out) return -1;
    DevBuf in[4], o;
    const uint32_t *host[4] = {a, b, c, d};
    hipError_t e;
    for (int k = 0; k < 4; ++k) {
        MCM_TRY(hipMalloc(&in[k].p, n * sizeof(uint32_t)));
        MCM_TRY(hipMemcpy(in[k].p, host[k], n * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    MCM_TRY(hipMalloc(&o.p, 7 * n * sizeof(double)));
    MCM_TRY(hipMemset(o.p, 0xFF, 7 * n * sizeof(double)));  // NaNs where nothing is written
    double *po = (double *)o.p;
    hipLaunchKernelGGL(noise_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, n, (const uint32_t *)in[0].p,
                       (const uint32_t *)in[1].p, (const uint32_t *)in[2].p, (const uint32_t *)in[3].p, po, po + n,
                       po + 2 * n, po + 3 * n, po + 4 * n, po + 5 * n, po + 6 * n);
    MCM_TRY(hipGetLastError());
    MCM_TRY(hipDeviceSynchronize());
    MCM_TRY(hipMemcpy(out, o.p, 7 * n * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int qpd_mcm_philox(int nk, int nc, const uint32_t *keys, const uint32_t *ctr, uint32_t *out) {
    if (nk < 1 || nk > (1 << 16) || nc < 1 || nc > (1 << 16) || !keys || !ctr || !out) return -1;
    const size_t words = 4 * (size_t)nk * nc;
    DevBuf dk, dc, dout;
    hipError_t e;
    MCM_TRY(hipMalloc(&dk.p, 2 * (size_t)nk * sizeof(uint32_t)));
    MCM_TRY(hipMalloc(&dc.p, words * sizeof(uint32_t)));
    MCM_TRY(hipMalloc(&dout.p, words * sizeof(uint32_t)));
    MCM_TRY(hipMemcpy(dk.p, keys, 2 * (size_t)nk * sizeof(uint32_t), hipMemcpyHostToDevice));
    MCM_TRY(hipMemcpy(dc.p, ctr, words * sizeof(uint32_t), hipMemcpyHostToDevice));
    MCM_TRY(hipMemset(dout.p, 0, words * sizeof(uint32_t)));
    hipLaunchKernelGGL(philox_kernel, dim3(nk), dim3(64), 0, nullptr, nc, (const uint32_t *)dk.p, (const uint32_t *)dc.p,
                       (uint32_t *)dout.p);
    MCM_TRY(hipGetLastError());
    MCM_TRY(hipDeviceSynchronize());
    MCM_TRY(hipMemcpy(out, dout.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

#undef MCM_TRY

}  // extern "C"
