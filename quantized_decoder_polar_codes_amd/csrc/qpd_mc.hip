// qpd_mc.hip -- GPU-resident Monte-Carlo front end.
//
// Replaces the reference driver's per-frame Python loop
// (mainQuantizedDecoder_LLRDomain.py:151-176): message bits, optional CRC
// (CRCEnc, :153-156), polar encoding (the un-vendored PolarEnc, restated:
// u[info] = msg, x = u F^{(x)n} in natural order), BPSK, AWGN in float64
// (`y = bpsk + normal(0, sigma)`, `llr = y * 2 / sigma**2`, :161-165, no fused
// multiply-add; the division by sigma**2 is a multiplication by its reciprocal,
// within an ulp of the driver's quotient) and the driver's channel quantizer
// (saturate at the outer edges, else channel_lut[bisect_left(edges[:-1], llr) - 1],
// :167-176).
//
// Every random number is a pure function of (seed, GLOBAL frame id, word):
// Philox4x32-10 with counter = (frame_lo, frame_hi, word, stream tag), so a
// frame's content does not depend on batch size, grid, or how frames are
// sharded across GPUs -- the 1/2/4/8-GPU runs of one frame range see the same
// frames.  Gaussians: Box-Muller in float64 on 52-bit
// uniforms (two Philox words each), u1 in (0, 1], u2 in [0, 1).
//
// bisect_left is exact for any ascending edges: a guess from the mean bin
// width, checked against its two neighbouring edges (one LDS read); only a
// wrong guess walks, and the walk ends at the first edge >= llr whatever the
// guess (uniform edges, the driver's linspace, are almost never wrong).
//
// PRE mode (qpd_mc_decode): the frame's symbols are staged in LDS and the
// kernel writes the decoder's root pre-pass row instead (root_pre_kernel,
// qpd_fast.hip), so generation feeds the decode kernel directly: no int32
// symbols (4 KB per frame at N = 1024) written to HBM and read back.
//
// Work mapping: one wave per frame (grid-stride).  The frame's bits are
// handled bit-packed (32 positions per dword): lane d draws message dword d,
// the CRC is a table XOR (the register is linear in the message bits), the
// info bits are deposited into u words by the per-word info masks, and the
// encoder runs 5 in-word butterfly stages as shift/mask XORs plus log2(N/32)
// word stages in LDS.  Noise, LLR and quantizer: one position pair per lane
// and round, stored as int2 (512 B per wave-instruction, coalesced).
//
// LLR modes (qpd_mc_llr, qpd_mc_decode_f64): the frame's N float64 LLRs instead
// of symbols, row-major [B][N] -- the very doubles the symbol mode bisects, so
// quantizing them on the host gives its symbols bit for bit.  One 16-byte store
// per lane (1 KB of consecutive bytes per wave-instruction); two 8-byte stores
// from a base that is only 8-byte aligned (N is even: every row keeps the
// base's alignment).  MC_LLR compiles the quantizer and its LDS tables out;
// MC_LLR_REC runs it and stores rec[symbol], the continuous-domain driver's
// channel quantizer (mainQuantizedDecoder_ContinuousDomain.py) in this
// library's edge convention, saturations included.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "qpd_mc_core.hpp"

namespace qpd {

// (QPD_MC_PAIRS and QPD_MC_WPE, the generator's two tuning switches: qpd_mc_core.hpp,
// with the Philox / log / sincos functions, the deposit and butterfly block and the
// noise pair, which the transmit kernels of qpd_tx.hip share.  The LLR and quantizer
// step stays written out below: as a shared function, mc_llr_symbol there, it
// changes this kernel's register allocation -- profiles/AB_RECORDS.md.)
// What the generator writes per frame: int32 symbols, the root pre-pass row,
// the float64 LLRs, or the reconstruction values of the LLRs' symbols.
// MC_PRE_LO: the pre-pass row in lookup order (FastHostPlan::row_lo; root_pre_kernel<In, true>)
enum McMode { MC_SYM = 0, MC_PRE = 1, MC_LLR = 2, MC_LLR_REC = 3, MC_PRE_LO = 4 };
template <int MODE>
__global__ __launch_bounds__(64, QPD_MC_WPE) void mc_frames_kernel(McChannel C, int64_t frame0, int64_t B,
                                                       uint8_t *__restrict__ msg_out, int32_t *__restrict__ sym_out) {
#pragma clang fp contract(off)
    extern __shared__ uint32_t lds_mc[];
    constexpr bool PRE = MODE == MC_PRE || MODE == MC_PRE_LO, LO = MODE == MC_PRE_LO;
    constexpr bool LLR = MODE == MC_LLR || MODE == MC_LLR_REC;  // sym_out holds doubles, N per frame
    constexpr bool QUANT = MODE != MC_LLR;                      // the channel quantizer runs
    // PRE: sym_out holds pre-pass rows (N/4 dwords per frame), see McChannel
    uint32_t Tf = 0, Tg = 0;
    if (PRE) {
        Tf = C.f_tab[threadIdx.x & 31];
        Tg = C.g_tab[threadIdx.x];
    }
    const int t = threadIdx.x;
    const int N = C.N, K = C.K, A = C.A, M = C.n_edges - 1;
    const int nw = (N + 31) >> 5;        // u / x words
    const int kw = (K + 31) >> 5;        // information-bit words (message + CRC)
    // E[0] = -inf, E[1 + i] = edges[i]: E[lo] = edges[lo - 1] and E[lo + 1] = edges[lo] need no guards
    double *E = reinterpret_cast<double *>(lds_mc);
    double *rec = E + kMcMaxEdges + 1;  // MC_LLR_REC: [kMcMaxEdges - 1]
    int32_t *lut = reinterpret_cast<int32_t *>(rec + (MODE == MC_LLR_REC ? kMcMaxEdges - 1 : 0));
    uint32_t *xw = QUANT ? reinterpret_cast<uint32_t *>(lut + kMcMaxEdges) : lds_mc;  // MC_LLR: no tables
    uint32_t *bw = xw + nw;               // message + CRC bits (kw + 2 words)
    uint8_t *sy = reinterpret_cast<uint8_t *>(bw + kw + 2);  // PRE: the frame's N channel symbols
    if constexpr (QUANT) {
        for (int i = t; i < C.n_edges; i += 64) E[1 + i] = C.edges[i];
        if (t == 0) E[0] = -__builtin_inf();
        for (int i = t; i < M; i += 64) lut[i] = C.lut[i];
    }
    if constexpr (MODE == MC_LLR_REC)
        for (int i = t; i < C.q; i += 64) rec[i] = C.rec[i];
    const double lo_edge = QUANT ? C.edges[0] : 0.0, hi_edge = QUANT ? C.edges[M] : 0.0;
    const bool al16 = ((uintptr_t)sym_out & 15u) == 0;  // LLR: one 16-byte store per lane
    const double inv_w = hi_edge > lo_edge ? M / (hi_edge - lo_edge) : 0.0;
    for (int64_t f = blockIdx.x; f < B; f += gridDim.x) {
        const uint64_t gid = (uint64_t)(frame0 + f);
        const uint32_t glo = (uint32_t)gid, ghi = (uint32_t)(gid >> 32);
        // message dword d = Philox(w = d / 4).v[d % 4]; bits >= A cleared
        uint32_t crc_part = 0;
        for (int d = t; d < kw + 2; d += 64) {  // + 2 zero words: funnel reads past the last
            uint32_t m = 0;
            if (32 * d < A) {
                const Philox4 r = philox4x32_10(glo, ghi, (uint32_t)(d >> 2), kTagMsg, C.seed_lo, C.seed_hi);
                // r.v[d & 3] as selects (a dynamic index would go through scratch)
                const uint32_t lo2 = (d & 1) ? r.v[1] : r.v[0], hi2 = (d & 1) ? r.v[3] : r.v[2];
                m = (d & 2) ? hi2 : lo2;
                if (A - 32 * d < 32) m &= (1u << (A - 32 * d)) - 1u;
                // msg bytes 32d .. 32d+31 (A % 8 == 0: 8 B stores)
                uint8_t *mo = msg_out + f * A + 32 * d;
                const int nb = min(32, A - 32 * d);
                if ((A & 7) == 0 && nb == 32) {
                    uint32_t w4[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        const uint32_t nib = (m >> (4 * k)) & 0xFu;
                        w4[k] = (nib & 1u) | ((nib & 2u) << 7) | ((nib & 4u) << 14) | ((nib & 8u) << 21);
                    }
                    uint2 *o2 = reinterpret_cast<uint2 *>(mo);
#pragma unroll
                    for (int k = 0; k < 4; ++k) o2[k] = make_uint2(w4[2 * k], w4[2 * k + 1]);
                } else {
                    for (int b = 0; b < nb; ++b) mo[b] = (uint8_t)((m >> b) & 1u);
                }
                if (C.crc_n > 0)
                    for (uint32_t mm = m; mm; mm &= mm - 1u) crc_part ^= C.crc_tab[32 * d + __builtin_ctz(mm)];
            }
            bw[d] = m;
        }
        if (C.crc_n > 0) {  // CRC::encoding (utils.cpp:77-92): XOR of the set bits' contributions
            for (int s = 32; s >= 1; s >>= 1) crc_part ^= (uint32_t)__shfl_xor((int)crc_part, s, 64);
            __syncthreads();
            if (t == 0)
                for (int j = 0; j < K - A; ++j) {
                    const uint32_t bit = (crc_part >> (C.crc_n - 1 - j)) & 1u;
                    bw[(A + j) >> 5] |= bit << ((A + j) & 31);
                }
        }
        __syncthreads();
        // the deposit, the 5 in-word stages and the word stages of x = u F^{(x)n} (qpd_mc_core.hpp)
        mc_encode_words(C, t, nw, bw, xw);
        // AWGN + LLR + channel quantizer, positions 2p and 2p+1, QPD_MC_PAIRS
        // pairs per lane and round (p, p + 64, ...): their Philox / log / sincos
        // chains are independent straight-line code the scheduler interleaves
        auto noise = [&](int p, double (&nz)[2]) { mc_noise_pair(C, glo, ghi, p, nz); };
        auto quantize = [&](int p, const double (&nz)[2]) {
            const uint32_t xbits = xw[(2 * p) >> 5] >> ((2 * p) & 31);
            int s_out[2];
            double l_out[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const double bpsk = (xbits >> h) & 1u ? -1.0 : 1.0;
                const double y = bpsk + C.sigma * nz[h];
                const double llr = y * 2.0 * C.inv_s2;
                if constexpr (QUANT) {
                    // bisect_left over edges[0..M-1] for lo_edge < llr < hi_edge: lo in [1, M]
                    // with edges[lo - 1] < llr <= edges[lo]; guessed, checked, walked if wrong
                    const bool inner = llr > lo_edge && llr < hi_edge;
                    const double gi = fmin(fmax((llr - lo_edge) * inv_w + 1.0, 1.0), (double)M);
                    int lo = (int)gi;
                    if (inner && !(E[lo] < llr && llr <= E[lo + 1])) {
                        while (E[lo] >= llr) --lo;     // stops at lo >= 1: E[1] = lo_edge < llr
                        while (E[lo + 1] < llr) ++lo;  // stops at lo <= M: E[M + 1] = hi_edge > llr
                    }
                    const int sl = lut[lo - 1];
                    s_out[h] = inner ? sl : (llr <= lo_edge ? 0 : C.q - 1);
                }
                if constexpr (MODE == MC_LLR) l_out[h] = llr;
                if constexpr (MODE == MC_LLR_REC) l_out[h] = rec[s_out[h]];
            }
            if constexpr (LLR) {
                double *o = reinterpret_cast<double *>(sym_out) + f * N + 2 * p;
                if (al16) {
                    // a native vector, stored whole (a double2 struct's store is split into its fields)
                    typedef double f64x2 __attribute__((ext_vector_type(2)));
                    *reinterpret_cast<f64x2 *>(o) = f64x2{l_out[0], l_out[1]};
                } else {
                    o[0] = l_out[0];
                    o[1] = l_out[1];
                }
            } else if (PRE)
                *reinterpret_cast<uint16_t *>(sy + 2 * p) = (uint16_t)(s_out[0] | (s_out[1] << 8));
            else
                *reinterpret_cast<int2 *>(sym_out + f * N + 2 * p) = make_int2(s_out[0], s_out[1]);
        };
        for (int p0 = 0; 2 * p0 < N; p0 += 64 * QPD_MC_PAIRS) {
            double nz[QPD_MC_PAIRS][2];
#pragma unroll
            for (int i = 0; i < QPD_MC_PAIRS; ++i) noise(p0 + 64 * i + t, nz[i]);
#pragma unroll
            for (int i = 0; i < QPD_MC_PAIRS; ++i)
                if (2 * (p0 + 64 * i + t) < N) quantize(p0 + 64 * i + t, nz[i]);
        }
        __syncthreads();
        if (PRE) {
            // root_pre_kernel's row from the staged symbols: word w of f(y),
            // g(y, 0), g(y, 1) from symbols [8w, 8w+8) and [N/2 + 8w, ...);
            // whole waves stay active through the lookups (inactive lanes
            // would read 0 from the table registers)
            const int nwh = N >> 4;  // words per segment (N >= 16)
            uint32_t *row = reinterpret_cast<uint32_t *>(sym_out) + f * (N >> 2);
            for (int w0 = 0; w0 < nwh; w0 += 64) {
                const int w = min(w0 + t, nwh - 1);
                uint32_t a = 0, b = 0;
                for (int i = 0; i < 8; ++i) {
                    if constexpr (LO) {  // the runs of four symbols at 4w and N/4 + 4w of each half (root_pre_kernel)
                        const int e = 4 * w + (i < 4 ? i : (N >> 2) + i - 4);
                        a |= (uint32_t)sy[e] << (4 * i);
                        b |= (uint32_t)sy[(N >> 1) + e] << (4 * i);
                        continue;
                    }
                    a |= (uint32_t)sy[8 * w + i] << (4 * i);
                    b |= (uint32_t)sy[(N >> 1) + 8 * w + i] << (4 * i);
                }
                const uint32_t fw = lut_vec<8, LO>(Tf, a, b, 0u);
                const uint32_t g0 = lut_vec<8, LO>(Tg, a, b, 0u);
                const uint32_t g1 = lut_vec<8, LO>(Tg, a, b, 0xFFu);
                if (w0 + t < nwh) {
                    row[w] = fw;
                    row[nwh + w] = g0;
                    row[2 * nwh + w] = g1;
                }
            }
            __syncthreads();
        }
    }
}

// Bit and block errors of decoded frames against their messages, added to
// counts[0] / counts[1] (the driver's counters, mainQuantizedDecoder_LLRDomain.py:181-183):
// one wave per frame (grid-stride, four frames' loads in flight per wave), 8
// bytes per lane per step -- the bytes are 0 / 1, so popcount(a ^ b) counts the
// differing ones; a frame's block error is one ballot, the bit errors are
// reduced once per wave; two atomics per wave.
__global__ __launch_bounds__(256) void mc_count_kernel(const uint8_t *__restrict__ bits,
                                                       const uint8_t *__restrict__ msg, int64_t B, int K,
                                                       unsigned long long *__restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t waves = (int64_t)gridDim.x * (blockDim.x >> 6);
    unsigned be = 0, fe = 0;  // be: this lane's share of the bit errors
    const bool vec = (K & 7) == 0 && ((uintptr_t)bits & 7) == 0 && ((uintptr_t)msg & 7) == 0;
    if (vec && K <= 512) {  // one 8-byte step per lane covers a frame
        const bool on = 8 * lane < K;
        for (int64_t f0 = wave; f0 < B; f0 += 4 * waves) {
            unsigned long long x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t f = f0 + u * waves;
                x[u] = 0;
                if (f < B && on)
                    x[u] = *(const unsigned long long *)(bits + f * K + 8 * lane) ^
                           *(const unsigned long long *)(msg + f * K + 8 * lane);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                be += __popcll(x[u]);
                fe += __ballot(x[u] != 0) != 0;
            }
        }
    } else {
        for (int64_t f = wave; f < B; f += waves) {
            const uint8_t *a = bits + f * K, *b = msg + f * K;
            unsigned e = 0;
            if (vec) {
                for (int i = 8 * lane; i < K; i += 512)
                    e += __popcll(*(const unsigned long long *)(a + i) ^ *(const unsigned long long *)(b + i));
            } else {
                for (int i = lane; i < K; i += 64) e += (a[i] ^ b[i]) & 1u;
            }
            be += e;
            fe += __ballot(e != 0) != 0;
        }
    }
    for (int m = 32; m >= 1; m >>= 1) be += (unsigned)__shfl_xor((int)be, m, 64);
    if (lane == 0 && be) {
        atomicAdd(counts, (unsigned long long)be);
        atomicAdd(counts + 1, (unsigned long long)fe);
    }
}

// Dynamic LDS of mc_frames_kernel<mode>: the quantizer's tables (none in
// MC_LLR; the reconstruction values too in MC_LLR_REC), the frame's bit words,
// the staged symbols (MC_PRE).
inline size_t mc_lds_bytes(int N, int K, int mode) {
    const size_t tables = mode == MC_LLR ? 0
                                         : (kMcMaxEdges + 1) * sizeof(double) + kMcMaxEdges * sizeof(int32_t) +
                                               (mode == MC_LLR_REC ? (kMcMaxEdges - 1) * sizeof(double) : 0);
    return tables + 4 * (((N + 31) >> 5) + ((K + 31) >> 5) + 2) + (mode == MC_PRE || mode == MC_PRE_LO ? (size_t)N : 0);
}

}  // namespace qpd
