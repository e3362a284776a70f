// qpd_llr_quant.hpp -- the driver's channel quantizer for one LLR
// (mainQuantizedDecoder_LLRDomain.py:167-176): saturate at the outer edges,
//     llr <= edges[0] -> 0,   llr >= edges[M] -> q - 1,
// else channel_lut[bisect_left(edges[:M], llr) - 1].  One text for the front
// kernel (qpd_llr.hip), the host-buffer entry point (qpd_capi_llr.hpp) and the
// native check (tests/native/llr_quant_check.cpp); no HIP needed (g++ builds it).
//
// The edges are read in the guard layout of mc_frames_kernel:
//     E[0] = -inf,  E[1 + i] = edges[i]  (i <= M),
// so E[lo] = edges[lo - 1] and E[lo + 1] = edges[lo] need no bounds test.
// bisect_left is exact for any ascending edges, duplicates included: a guess
// from the mean bin width, checked against its two neighbouring edges; only a
// wrong guess walks, and the walk ends at the one lo in [1, M] with
// E[lo] < llr <= E[lo + 1] whatever the guess was.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define QPD_HD __host__ __device__ __forceinline__
#else
#define QPD_HD inline
#endif

namespace qpd {

constexpr int kLlrMaxEdges = 257;  // channel quantizer with up to 256 bins (qpd_mc.hip: kMcMaxEdges)

// What the quantizer needs besides its tables.
struct LlrQuant {
    int32_t M, q;           // bins (n_edges - 1), channel symbols
    double lo_edge, hi_edge;  // edges[0], edges[M]
    double inv_w;           // M / (hi_edge - lo_edge): bins per LLR unit (0 where that is not finite and positive)
};

QPD_HD LlrQuant llr_quant_params(const double *edges, int n_edges, int q) {
    LlrQuant Q;
    Q.M = n_edges - 1;
    Q.q = q;
    Q.lo_edge = edges[0];
    Q.hi_edge = edges[Q.M];
    const double w = Q.hi_edge - Q.lo_edge;
    Q.inv_w = (w > 0 && w <= 1.7976931348623157e308) ? Q.M / w : 0.0;
    return Q;
}

// E[0 .. M + 1] from edges[0 .. M] (host side; the kernel stages it in LDS).
inline void llr_guard_edges(const double *edges, int n_edges, double *E) {
    E[0] = -__builtin_inf();
    for (int i = 0; i < n_edges; ++i) E[1 + i] = edges[i];
}

// The symbol of one LLR; -1 for a NaN, which has no symbol in the driver.
// E: guard layout [M + 2]; lut: [M] entries in [0, q) (any integer type).
template <class Lut>
QPD_HD int quantize_llr(double llr, const LlrQuant &Q, const double *E, const Lut *lut) {
    if (llr != llr) return -1;
    if (llr <= Q.lo_edge) return 0;
    if (llr >= Q.hi_edge) return Q.q - 1;
    // lo_edge < llr < hi_edge: lo in [1, M].  The guess is clamped with comparisons that
    // drop a NaN (inf * 0 where an outer edge is infinite), so it is always a valid index.
    double gi = (llr - Q.lo_edge) * Q.inv_w + 1.0;
    gi = gi >= 1.0 ? gi : 1.0;
    gi = gi <= (double)Q.M ? gi : (double)Q.M;
    int lo = (int)gi;
    if (!(E[lo] < llr && llr <= E[lo + 1])) {
        while (E[lo] >= llr) --lo;     // stops at lo >= 1: E[1] = lo_edge < llr
        while (E[lo + 1] < llr) ++lo;  // stops at lo <= M: E[M + 1] = hi_edge > llr
    }
    return (int)lut[lo - 1];
}

}  // namespace qpd
