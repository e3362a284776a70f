// qpd_llr.hip -- the channel quantizer on the device: float64 / float32 LLRs in,
// what a LUT decoder reads out (qpd_quantize_llr, qpd_decode_llr).
//
// The rule is the driver's (mainQuantizedDecoder_LLRDomain.py:167-176), one
// shared text (qpd_llr_quant.hpp); a float32 LLR is widened to double first,
// which is exact.  A NaN has no symbol there: it becomes symbol 0 and raises the
// decoder's error word (ERR_NAN_LLR).
//
// One kernel template over the input type and three output forms:
//   LLR_PRE  the decoder's root pre-pass row, root_pre_kernel's layout
//            (qpd_fast_pre.hpp: f(y) | g(y, 0) | g(y, 1), N/16 nibble words each):
//            the kernel takes the pre-pass's place, no symbol touches HBM.
//            One thread per output word, as there: it owns LLRs [8w, 8w + 8) and
//            [N/2 + 8w, N/2 + 8w + 8) of its frame.
//   LLR_I32  int32 symbols into the decoder's staging chunk (every decoder
//            without a pre-pass), row-major, one 16-byte load per thread and step.
//   LLR_U8   uint8 symbols (qpd_quantize_llr), the same mapping.
//
// LLR_PRE reads its 2 x 8 LLRs in one of two ways (COOP):
//   false  the owner reads them itself, 16 bytes per load: the lanes of one load
//          are 64 (float64) or 32 (float32) bytes apart;
//   true   the block's 256 words are read cooperatively -- lane l of a load takes
//          the l-th 16 bytes of the words' LLRs, consecutive lanes consecutive
//          addresses -- quantized where they land and handed to their owners as
//          bytes through LDS (4 KB per block, two barriers per 256 words).
// Both compute the same rows (tests/test_gpu_llr_input.py runs both); DESIGN.md
// records what each measured.
//
// The edges sit in LDS in the guard layout (E[0] = -inf), with the lut as bytes
// and, for LLR_PRE, the root's f / g tables as bytes (stage_tab).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qpd_fast_lookup.hpp"
#include "qpd_llr_quant.hpp"
#include "qpd_types.hpp"

namespace qpd {

// LLR_PRE_LO: the pre-pass row in lookup order (FastHostPlan::row_lo; root_pre_kernel<In, true>)
enum LlrOut { LLR_PRE = 0, LLR_I32 = 1, LLR_U8 = 2, LLR_PRE_LO = 3 };

struct LlrFront {
    LlrQuant Q;
    int32_t N, n;      // code length and its log2
    int32_t vec;       // the LLR base is 16-byte aligned: vector loads
    int32_t out_vec;   // LLR_U8: the symbol base allows the vector store of one step
    const uint32_t *f_tab, *g_tab;  // LLR_PRE: node 0's nibble tables (FastPlan f_tab / g_tab)
    int32_t *err;
    double edges[kLlrMaxEdges];     // [M + 1], ascending (kernel arguments; staged in LDS)
    uint8_t lut[kLlrMaxEdges - 1];  // [M], values in [0, q)
};

template <class T>
struct LlrVec;
template <>
struct LlrVec<double> {
    typedef double type __attribute__((ext_vector_type(2)));
};
template <>
struct LlrVec<float> {
    typedef float type __attribute__((ext_vector_type(4)));
};

// EPL LLRs from p (EPL * sizeof(T) = 16): one 16-byte load, or scalar loads.
template <class T, int EPL>
__device__ __forceinline__ void llr_load(const T *p, bool vec, double (&x)[EPL]) {
    if (vec) {
        const typename LlrVec<T>::type v = *reinterpret_cast<const typename LlrVec<T>::type *>(p);
#pragma unroll
        for (int k = 0; k < EPL; ++k) x[k] = (double)v[k];
    } else {
#pragma unroll
        for (int k = 0; k < EPL; ++k) x[k] = (double)p[k];
    }
}

// One LLR's symbol; a NaN: 0, and `nan` set.
__device__ __forceinline__ uint32_t llr_sym(double x, const LlrQuant &Q, const double *E, const uint8_t *lut, uint32_t &nan) {
    const int s = quantize_llr(x, Q, E, lut);
    nan |= (uint32_t)(s < 0);
    return s < 0 ? 0u : (uint32_t)s;
}

template <class T, int OUT_, bool COOP>
__global__ __launch_bounds__(256) void llr_front_kernel(LlrFront C, const T *__restrict__ in, int64_t B,
                                                        void *__restrict__ out) {
    // LO: word w's eight `a` symbols are the runs at 4w and N/4 + 4w of the row's first half, its `b`
    // symbols the same of the second half, and lookup k lands at nibble il_nib<8>(k)
    constexpr bool LO = OUT_ == LLR_PRE_LO;
    constexpr int OUT = LO ? (int)LLR_PRE : OUT_;
    constexpr int EPL = 16 / (int)sizeof(T);  // LLRs per 16-byte load: 2 or 4
    __shared__ __attribute__((aligned(16))) double E[kLlrMaxEdges + 1];
    __shared__ __attribute__((aligned(16))) uint8_t lut[kLlrMaxEdges - 1];
    __shared__ __attribute__((aligned(16))) uint8_t tf[OUT == LLR_PRE ? 256 : 8], tg[OUT == LLR_PRE ? 512 : 8];
    __shared__ __attribute__((aligned(16))) uint8_t sy[OUT == LLR_PRE && COOP ? 4096 : 8];
    const int tid = threadIdx.x;
    const LlrQuant Q = C.Q;
    for (int i = tid; i <= Q.M; i += 256) E[1 + i] = C.edges[i];
    if (tid == 0) E[0] = -__builtin_inf();
    for (int i = tid; i < Q.M; i += 256) lut[i] = C.lut[i];
    if constexpr (OUT == LLR_PRE) {
        if (tid < 64) {  // node 0 (posi 0), as root_pre_kernel
            stage_tab(tg, C.g_tab[tid], tid);
            if (tid < 32) stage_tab(tf, C.f_tab[tid], tid);
        }
    }
    __syncthreads();
    const bool vec = C.vec != 0;
    uint32_t nan = 0;
    if constexpr (OUT == LLR_PRE) {
        const int wsh = C.n - 4;  // log2 words per segment (N >= 16)
        const int half = C.N >> 1;
        const int64_t total = B << wsh;
        uint32_t *pre = reinterpret_cast<uint32_t *>(out);
        for (int64_t base = (int64_t)blockIdx.x * 256; base < total; base += (int64_t)gridDim.x * 256) {
            const int64_t t0 = base + tid;
            const int64_t t = t0 < total ? t0 : total - 1;
            const int64_t f = t >> wsh;
            const int w = (int)(t & ((1 << wsh) - 1));
            uint32_t a = 0, b = 0;  // eight nibble symbols of each half
            if constexpr (COOP) {
                constexpr int LPW = 8 / EPL;  // lanes per word and half, and loads per thread and half
                double x[2 * LPW][EPL];
#pragma unroll
                for (int i = 0; i < 2 * LPW; ++i) {
                    const int p = (i % LPW) * 256 + tid, u = p / LPW;
                    const int64_t tu = base + u < total ? base + u : total - 1;
                    const T *src = in + ((tu >> wsh) << C.n) + (i / LPW) * half + 8 * (int)(tu & ((1 << wsh) - 1)) +
                                   (p % LPW) * EPL;
                    if constexpr (LO) {  // symbols at .. at + EPL - 1 of word wu: the run at 4 wu, or at N/4 + 4 wu
                        const int wu = (int)(tu & ((1 << wsh) - 1)), at = (p % LPW) * EPL;
                        src = in + ((tu >> wsh) << C.n) + (i / LPW) * half + 4 * wu + (at < 4 ? at : (half >> 1) + at - 4);
                    }
                    llr_load<T, EPL>(src, vec, x[i]);
                }
#pragma unroll
                for (int i = 0; i < 2 * LPW; ++i) {
                    const int p = (i % LPW) * 256 + tid;
                    uint32_t s = 0;
#pragma unroll
                    for (int k = 0; k < EPL; ++k) s |= llr_sym(x[i][k], Q, E, lut, nan) << (8 * k);
                    uint8_t *dst = sy + (i / LPW) * 2048 + p * EPL;  // word u = p / LPW, byte (p % LPW) * EPL
                    if constexpr (EPL == 2) *reinterpret_cast<uint16_t *>(dst) = (uint16_t)s;
                    else *reinterpret_cast<uint32_t *>(dst) = s;
                }
                __syncthreads();
                const uint2 a8 = *reinterpret_cast<const uint2 *>(sy + 8 * tid);
                const uint2 b8 = *reinterpret_cast<const uint2 *>(sy + 2048 + 8 * tid);
                a = nib_pack4(a8.x) | (nib_pack4(a8.y) << 16);
                b = nib_pack4(b8.x) | (nib_pack4(b8.y) << 16);
                __syncthreads();  // sy is rewritten by the next 256 words
            } else {
                const T *y = in + (f << C.n) + (LO ? 4 : 8) * w;
                double x[2][8 / EPL][EPL];
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int i = 0; i < 8 / EPL; ++i)
                        llr_load<T, EPL>(y + h * half + (LO && i * EPL >= 4 ? (half >> 1) + i * EPL - 4 : i * EPL), vec, x[h][i]);
#pragma unroll
                for (int i = 0; i < 8 / EPL; ++i)
#pragma unroll
                    for (int k = 0; k < EPL; ++k) {
                        a |= llr_sym(x[0][i][k], Q, E, lut, nan) << (4 * (i * EPL + k));
                        b |= llr_sym(x[1][i][k], Q, E, lut, nan) << (4 * (i * EPL + k));
                    }
            }
            // root_pre_kernel's lookups: byte j of X / Y is the index of element 2j / 2j + 1
            const uint32_t X = ((a << 4) & 0xF0F0F0F0u) | (b & 0x0F0F0F0Fu);
            const uint32_t Y = (a & 0xF0F0F0F0u) | ((b >> 4) & 0x0F0F0F0Fu);
            uint32_t fw = 0, g0 = 0, g1 = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t idx = __builtin_amdgcn_ubfe((k & 1) ? Y : X, 8 * (k >> 1), 8);
                const int nb = 4 * (LO ? il_nib<8>(k) : k);
                fw |= (uint32_t)tf[idx] << nb;
                g0 |= (uint32_t)tg[idx] << nb;
                g1 |= (uint32_t)tg[256 + idx] << nb;
            }
            if (t0 < total) {
                uint32_t *row = pre + (f << (C.n - 2));
                row[w] = fw;
                row[(1 << wsh) + w] = g0;
                row[(2 << wsh) + w] = g1;
            }
        }
    } else {
        // row-major symbols: groups of EPL LLRs, four groups per thread and round in flight
        const int64_t n = B << C.n, groups = n / EPL;
        const int64_t stride = (int64_t)gridDim.x * 256;
        for (int64_t g0 = (int64_t)blockIdx.x * 256 + tid; g0 < groups; g0 += 4 * stride) {
            double x[4][EPL];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t g = g0 + r * stride;
                if (g < groups) llr_load<T, EPL>(in + g * EPL, vec, x[r]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t g = g0 + r * stride;
                if (g >= groups) continue;
                uint32_t s[EPL];
#pragma unroll
                for (int k = 0; k < EPL; ++k) s[k] = llr_sym(x[r][k], Q, E, lut, nan);
                if constexpr (OUT == LLR_I32) {  // the staging chunk: 16-byte aligned, g * EPL * 4 a multiple of 8 / 16
                    int32_t *o = reinterpret_cast<int32_t *>(out) + g * EPL;
                    if constexpr (EPL == 2) *reinterpret_cast<int2 *>(o) = make_int2((int)s[0], (int)s[1]);
                    else *reinterpret_cast<int4 *>(o) = make_int4((int)s[0], (int)s[1], (int)s[2], (int)s[3]);
                } else {
                    uint8_t *o = reinterpret_cast<uint8_t *>(out) + g * EPL;
                    if (C.out_vec) {
                        if constexpr (EPL == 2) *reinterpret_cast<uint16_t *>(o) = (uint16_t)(s[0] | (s[1] << 8));
                        else *reinterpret_cast<uint32_t *>(o) = s[0] | (s[1] << 8) | (s[2] << 16) | (s[3] << 24);
                    } else {
#pragma unroll
                        for (int k = 0; k < EPL; ++k) o[k] = (uint8_t)s[k];
                    }
                }
            }
        }
        // float32: up to three LLRs after the last whole group (B * N is even)
        for (int64_t i = groups * EPL + (int64_t)blockIdx.x * 256 + tid; i < n; i += stride) {
            const uint32_t s = llr_sym((double)in[i], Q, E, lut, nan);
            if constexpr (OUT == LLR_I32) reinterpret_cast<int32_t *>(out)[i] = (int)s;
            else reinterpret_cast<uint8_t *>(out)[i] = (uint8_t)s;
        }
    }
    if (nan) atomicOr(C.err, (int)ERR_NAN_LLR);
}

}  // namespace qpd
