// qpd_tx.hip -- the transmit side for caller-chosen messages (qpd_encode,
// qpd_tx_frames; include/qpd.h): what mc_frames_kernel (qpd_mc.hip) does for the
// messages it draws, with the message read from the caller's buffer instead, the
// CRC's tail optionally scrambled by a mask (an RNTI), and the information bits
// and the codeword as outputs.  A unit of its own (build.py UNITS): the
// generator's instantiations stay in qpd_capi.hip's unit, and both take the
// Philox / Box-Muller / deposit / butterfly / quantizer code from qpd_mc_core.hpp.
//
// Replaces PolarBDEnc.Encoder.PolarEnc / CRCEnc of the reference drivers
// (mainQuantizedDecoder_LLRDomain.py:10-11, :72-73, :153-158; the package is not
// part of the reference) batched, and the drivers' channel (:161-176) behind it.
//
// Work mapping: the generator's -- one wave per frame, grid-stride.  Lane d
// packs message bytes 32d .. 32d+31 into message dword d (four 8-byte loads where
// the rows are a multiple of 8 bytes on an 8-byte aligned base, else a byte
// loop), the inverse of the generator's nibble spread; a byte with a bit above
// bit 0 raises ERR_MSG_BIT in the decoder's error word, on a branch clean input
// never takes, and counts as its low bit.  Then the generator's CRC table XOR and
// wave reduction, the mask XORed onto the register, the deposit, 5 in-word stages
// and the word stages in LDS.
//   tx_encode_kernel: information bits and codeword unpacked, 32 bits to four
//     8-byte stores per lane (consecutive lanes, consecutive bytes), or bytes.
//   tx_frames_kernel: the generator's noise and quantizer loop on the codeword
//     words in LDS; no_signal skips the encoder and drops the BPSK term.
// LDS: the generator's dynamic layout (mc_lds_bytes of the matching mode).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qpd_mc_core.hpp"
#include "qpd_tx_kernels.hpp"
#include "qpd_types.hpp"

namespace qpd {

// Four 0/1 bytes of a dword -> a nibble (the inverse of the generator's spread).
__device__ __forceinline__ uint32_t tx_pack4(uint32_t w) {
    return (w & 1u) | ((w >> 7) & 2u) | ((w >> 14) & 4u) | ((w >> 21) & 8u);
}

// A nibble -> four 0/1 bytes (the generator's spread).
__device__ __forceinline__ uint32_t tx_spread4(uint32_t nib) {
    return (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
}

// One frame's information bits into bw[0 .. kw + 2) (LDS; the two words past the
// last are zero, the deposit's funnel reads them): the message row `row` ([A]
// bytes) packed, then for the CRC-aided kinds the first K - A bits of
// (check code ^ mask).  Ends with a barrier.  vec8: `row` is 8-byte aligned and A
// a multiple of 8.
__device__ __forceinline__ void tx_info_bits(const McChannel &C, const uint8_t *__restrict__ row, bool vec8, uint32_t mask,
                                             int32_t *err, int t, int kw, uint32_t *bw) {
    const int A = C.A, K = C.K;
    uint32_t crc_part = 0;
    for (int d = t; d < kw + 2; d += 64) {
        uint32_t m = 0;
        if (32 * d < A) {
            const uint8_t *mi = row + 32 * d;
            const int nb = min(32, A - 32 * d);
            uint32_t bad = 0;
            if (vec8 && nb == 32) {
                const uint2 *i2 = reinterpret_cast<const uint2 *>(mi);
                uint2 v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = i2[k];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    bad |= (v[k].x | v[k].y) & 0xFEFEFEFEu;
                    m |= (tx_pack4(v[k].x) | (tx_pack4(v[k].y) << 4)) << (8 * k);
                }
            } else {
                for (int b = 0; b < nb; ++b) {
                    const uint32_t by = mi[b];
                    bad |= by & 0xFEu;
                    m |= (by & 1u) << b;
                }
            }
            if (bad) atomicOr(err, (int)ERR_MSG_BIT);
            if (C.crc_n > 0)
                for (uint32_t mm = m; mm; mm &= mm - 1u) crc_part ^= C.crc_tab[32 * d + __builtin_ctz(mm)];
        }
        bw[d] = m;
    }
    if (C.crc_n > 0) {  // CRC::encoding (utils.cpp:77-92) as in mc_frames_kernel, then the mask on the register
        for (int s = 32; s >= 1; s >>= 1) crc_part ^= (uint32_t)__shfl_xor((int)crc_part, s, 64);
        crc_part ^= mask;
        __syncthreads();
        if (t == 0)
            for (int j = 0; j < K - A; ++j) {
                const uint32_t bit = (crc_part >> (C.crc_n - 1 - j)) & 1u;
                bw[(A + j) >> 5] |= bit << ((A + j) & 31);
            }
    }
    __syncthreads();
}

// `n` bits of the words w[] (LDS) as 0/1 bytes at out[0 .. n): lane t writes the
// bytes of word t, t + 64, ...  vec8: out is 8-byte aligned and n a multiple of 8.
__device__ __forceinline__ void tx_unpack_row(const uint32_t *w, int n, uint8_t *__restrict__ out, bool vec8, int t) {
    for (int d = t; 32 * d < n; d += 64) {
        const uint32_t m = w[d];
        const int nb = min(32, n - 32 * d);
        uint8_t *o = out + 32 * d;
        if (vec8 && nb == 32) {
            uint2 *o2 = reinterpret_cast<uint2 *>(o);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                o2[k] = make_uint2(tx_spread4((m >> (8 * k)) & 0xFu), tx_spread4((m >> (8 * k + 4)) & 0xFu));
        } else {
            for (int b = 0; b < nb; ++b) o[b] = (uint8_t)((m >> b) & 1u);
        }
    }
}

__global__ __launch_bounds__(64) void tx_encode_kernel(McChannel C, int64_t B, TxIo io) {
    extern __shared__ uint32_t lds_tx[];
    const int t = threadIdx.x;
    const int N = C.N, K = C.K, A = C.A;
    const int nw = (N + 31) >> 5, kw = (K + 31) >> 5;
    uint32_t *xw = lds_tx, *bw = xw + nw;
    const bool in8 = (A & 7) == 0 && ((uintptr_t)io.msg & 7u) == 0;
    const bool info8 = (K & 7) == 0 && ((uintptr_t)io.info & 7u) == 0;
    const bool cw8 = (N & 7) == 0 && ((uintptr_t)io.cw & 7u) == 0;
    for (int64_t f = blockIdx.x; f < B; f += gridDim.x) {
        tx_info_bits(C, io.msg + f * A, in8, io.mask, io.err, t, kw, bw);
        if (io.info) tx_unpack_row(bw, K, io.info + f * K, info8, t);
        if (io.cw) {
            mc_encode_words(C, t, nw, bw, xw);
            tx_unpack_row(xw, N, io.cw + f * N, cw8, t);
        }
        __syncthreads();  // the next frame overwrites bw / xw
    }
}

template <int OUT>
__global__ __launch_bounds__(64, QPD_MC_WPE) void tx_frames_kernel(McChannel C, int64_t frame0, int64_t B, TxIo io) {
#pragma clang fp contract(off)
    extern __shared__ uint32_t lds_tx[];
    constexpr bool LLR = OUT == TX_LLR || OUT == TX_LLR_REC;
    constexpr bool QUANT = OUT != TX_LLR;
    const int t = threadIdx.x;
    const int N = C.N, K = C.K, A = C.A, M = C.n_edges - 1;
    const int nw = (N + 31) >> 5, kw = (K + 31) >> 5;
    // the generator's layout: E[0] = -inf, E[1 + i] = edges[i]; rec; lut; the bit words
    double *E = reinterpret_cast<double *>(lds_tx);
    double *rec = E + kMcMaxEdges + 1;
    int32_t *lut = reinterpret_cast<int32_t *>(rec + (OUT == TX_LLR_REC ? kMcMaxEdges - 1 : 0));
    uint32_t *xw = QUANT ? reinterpret_cast<uint32_t *>(lut + kMcMaxEdges) : lds_tx;
    uint32_t *bw = xw + nw;
    if constexpr (QUANT) {
        for (int i = t; i < C.n_edges; i += 64) E[1 + i] = C.edges[i];
        if (t == 0) E[0] = -__builtin_inf();
        for (int i = t; i < M; i += 64) lut[i] = C.lut[i];
    }
    if constexpr (OUT == TX_LLR_REC)
        for (int i = t; i < C.q; i += 64) rec[i] = C.rec[i];
    const double lo_edge = QUANT ? C.edges[0] : 0.0, hi_edge = QUANT ? C.edges[M] : 0.0;
    const double inv_w = hi_edge > lo_edge ? M / (hi_edge - lo_edge) : 0.0;
    const bool in8 = (A & 7) == 0 && ((uintptr_t)io.msg & 7u) == 0;
    const bool nosig = io.no_signal != 0;
    const uintptr_t obase = (uintptr_t)io.frames;
    for (int i = t; i < nw; i += 64) xw[i] = 0;  // no_signal: the bits are not read into y, but the shifts read them
    __syncthreads();
    for (int64_t f = blockIdx.x; f < B; f += gridDim.x) {
        const uint64_t gid = (uint64_t)(frame0 + f);
        const uint32_t glo = (uint32_t)gid, ghi = (uint32_t)(gid >> 32);
        if (!nosig) {
            tx_info_bits(C, io.msg + f * A, in8, io.mask, io.err, t, kw, bw);
            mc_encode_words(C, t, nw, bw, xw);
        }
        for (int p = t; 2 * p < N; p += 64) {
            double nz[2];
            mc_noise_pair(C, glo, ghi, p, nz);
            const uint32_t xbits = xw[(2 * p) >> 5] >> ((2 * p) & 31);
            int s_out[2] = {0, 0};
            double l_out[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const double llr = mc_llr_symbol<QUANT>(C, (xbits >> h) & 1u, nosig, nz[h], E, lut, lo_edge, hi_edge, inv_w, M,
                                                        &s_out[h]);
                l_out[h] = OUT == TX_LLR_REC ? rec[s_out[h]] : llr;
            }
            if constexpr (LLR) {
                double *o = reinterpret_cast<double *>(io.frames) + f * N + 2 * p;
                if ((obase & 15u) == 0) {
                    typedef double f64x2 __attribute__((ext_vector_type(2)));
                    *reinterpret_cast<f64x2 *>(o) = f64x2{l_out[0], l_out[1]};
                } else {
                    o[0] = l_out[0];
                    o[1] = l_out[1];
                }
            } else if constexpr (OUT == TX_SYM_U8) {
                uint8_t *o = reinterpret_cast<uint8_t *>(io.frames) + f * N + 2 * p;
                if ((obase & 1u) == 0) {  // N is even: every pair keeps the base's parity
                    *reinterpret_cast<uint16_t *>(o) = (uint16_t)((s_out[0] & 0xFF) | ((s_out[1] & 0xFF) << 8));
                } else {
                    o[0] = (uint8_t)s_out[0];
                    o[1] = (uint8_t)s_out[1];
                }
            } else {
                int32_t *o = reinterpret_cast<int32_t *>(io.frames) + f * N + 2 * p;
                if ((obase & 7u) == 0) {
                    *reinterpret_cast<int2 *>(o) = make_int2(s_out[0], s_out[1]);
                } else {
                    o[0] = s_out[0];
                    o[1] = s_out[1];
                }
            }
        }
        __syncthreads();  // the next frame overwrites bw / xw
    }
}

const void *tx_encode_kernel_fn() { return reinterpret_cast<const void *>(&tx_encode_kernel); }

const void *tx_frames_kernel_fn(int out) {
    switch (out) {
        case TX_SYM_I32: return reinterpret_cast<const void *>(&tx_frames_kernel<TX_SYM_I32>);
        case TX_SYM_U8: return reinterpret_cast<const void *>(&tx_frames_kernel<TX_SYM_U8>);
        case TX_LLR: return reinterpret_cast<const void *>(&tx_frames_kernel<TX_LLR>);
        default: return reinterpret_cast<const void *>(&tx_frames_kernel<TX_LLR_REC>);
    }
}

}  // namespace qpd
