// qpd_mc_core.hpp -- the device code the frame generator (mc_frames_kernel,
// qpd_mc.hip) and the transmit kernels for caller-chosen messages (qpd_tx.hip)
// share: Philox4x32-10, the 52-bit uniforms, log and sincos of the Box-Muller
// step, the kernel argument block, and -- as functions inlined into both -- the
// deposit and butterfly block of the encoder and one noise pair; and one
// position's LLR and channel symbol (mc_llr_symbol) as the transmit kernels call
// it, the statements of the generator's quantize step, which stays written out
// there (qpd_mc.hip says why; tests/test_gpu_tx_frames.py holds the two bit for
// bit together).  The arithmetic is documented where it is used
// (qpd_mc.hip's header); tests/native/mc_math_harness.hip runs it alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace qpd {

constexpr int kMcMaxEdges = 257;  // channel quantizer with up to 256 bins
constexpr uint32_t kTagMsg = 0x4d534731u, kTagNoise = 0x4e4f4931u;

struct Philox4 {
    uint32_t v[4];
};

__device__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                  uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0;
        c1 = (uint32_t)p1;
        c2 = n2;
        c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
        // the round keys stay two SGPRs advanced per round (SALU) instead of
        // 20 hoisted loop invariants, which would spill the kernel's SGPRs
        asm volatile("" : "+s"(k0), "+s"(k1));
    }
    Philox4 o;
    o.v[0] = c0;
    o.v[1] = c1;
    o.v[2] = c2;
    o.v[3] = c3;
    return o;
}

struct McChannel {
    int32_t N, K, q, n_edges;
    int32_t A, crc_n;     // crc_n > 0: A message bits + first K-A bits of their CRC
    double sigma, inv_s2; // AWGN std and 1 / (sigma*sigma): llr = (2y) * inv_s2
    uint32_t seed_lo, seed_hi;
    const uint32_t *info_mask;  // [N/32] bit i of word w: position 32w+i is an information bit
    const int32_t *info_pref;   // [N/32] information bits before word w
    const uint32_t *crc_tab;    // [A] CRC register contribution of message bit j (CA kinds)
    double edges[kMcMaxEdges];  // [n_edges], ascending (kernel arguments; staged in LDS)
    int32_t lut[kMcMaxEdges - 1];
    // PRE mode (qpd_mc_decode on a fast-engine decoder in pre-mode): instead
    // of int32 symbols, each frame's root pre-pass row (root_pre_kernel's
    // layout: f(y), g(y, 0), g(y, 1) as nibble words, N/4 dwords per frame),
    // computed from the frame's symbols staged in LDS with the root's tables.
    // MC_LLR_REC: reconstruction value per symbol, [q] with q <= 256 (device;
    // staged in LDS).  In f_tab's place, which only PRE mode reads: the struct
    // keeps its size, and the other modes' kernel arguments their offsets.
    union {
        const uint32_t *f_tab;  // node 0's nibble tables (FastPlan f_tab / g_tab)
        const double *rec;
    };
    const uint32_t *g_tab;
};

// The double 1.m in [1, 2) whose 52 mantissa bits are (a >> 12) : b -- two
// Philox words; 2 - x is then uniform on (0, 1], x - 1 on [0, 1) (52-bit grid).
__device__ __host__ inline double mc_one_m(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(double, ((uint64_t)(0x3FF00000u | (a >> 12)) << 32) | b);
}

// One Horner step a * b + c with the constant c as an SGPR operand of a VOP3
// v_fma_f64: the compiler otherwise keeps the polynomial constants in VGPRs and
// evaluates every step as a copy + v_fmac_f64 (two VALU instructions instead
// of one plus two scalar moves).
__device__ __forceinline__ double hfma(double a, double b, double c) {
    double r;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c));
    return r;
}

// sin and cos of x in [0, 2 pi] for the Box-Muller angle: reduction by
// q = rint(x * 2/pi) against pi/2 in three parts (Cody-Waite), then the
// fdlibm kernel polynomials (__kernel_sin / __kernel_cos, |r| <= pi/4, < 1 ulp).
// The angle never needs the large-argument (Payne-Hanek) path a general
// libm sin/cos carries (scratch memory, registers).
__device__ inline void mc_sincos(double x, double *sn, double *cs) {
    const double q = rint(x * 0.63661977236758134308);  // 2/pi
    double r = fma(-q, 1.57079632673412561417e+00, x);
    r = fma(-q, 6.07710050630396597660e-11, r);
    r = fma(-q, 2.02226624879595063154e-21, r);
    const double z = r * r;
    const double ps = hfma(z, hfma(z, hfma(z, fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08),
                                           2.75573137070700676789e-06), -1.98412698298579493134e-04),
                           8.33333333332248946124e-03);
    const double sr = fma(r * z, hfma(z, ps, -1.66666666666666324348e-01), r);
    const double pc = z * hfma(z, hfma(z, hfma(z, hfma(z, fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09),
                                                      -2.75573143513906633035e-07), 2.48015872894767294178e-05),
                                         -1.38888888888741095749e-03), 4.16666666666666019037e-02);
    const double hz = 0.5 * z, w = 1.0 - hz;
    const double cr = w + (((1.0 - w) - hz) + z * pc);
    // quadrant q & 3: (sr, cr), (cr, -sr), (-sr, -cr), (-cr, sr) -- as selects
    const int qi = (int)q;
    const double s0 = (qi & 1) ? cr : sr, c0 = (qi & 1) ? sr : cr;
    *sn = (qi & 2) ? -s0 : s0;
    *cs = ((qi + 1) & 2) ? -c0 : c0;
}

// log(u) for u in (0, 1]: fdlibm's __ieee754_log (u = m 2^k with m in
// [sqrt(2)/2, sqrt(2)), f = m - 1, s = f / (2 + f), the Remez polynomial in
// s^2; < 1 ulp) with its one division as a Newton-refined reciprocal plus a
// residual correction -- s enters only through s (hfsq + R), an O(f^3) term.
// A third of the instructions of the double-double device log.
__device__ inline double mc_log(double u) {
    int k;
    double m = frexp(u, &k);  // [0.5, 1)
    if (m < 0.70710678118654752440) {
        m += m;
        --k;
    }
    const double f = m - 1.0, dd = 2.0 + f;
    double r = __builtin_amdgcn_rcp(dd);
    r = fma(fma(-dd, r, 1.0), r, r);
    r = fma(fma(-dd, r, 1.0), r, r);
    double s = f * r;
    s = fma(fma(-dd, s, f), r, s);
    const double z = s * s, w = z * z;
    // fdlibm's Horner steps as fused multiply-adds
    const double t1 = w * hfma(w, fma(w, 1.531383769920937332e-01, 2.222219843214978396e-01), 3.999999999940941908e-01);
    const double t2 = z * hfma(w, hfma(w, fma(w, 1.479819860511658591e-01, 1.818357216161805012e-01), 2.857142874366239149e-01),
                               6.666666666666735130e-01);
    const double R = t2 + t1, hfsq = 0.5 * f * f, dk = (double)k;
    return dk * 6.93147180369123816490e-01 - ((hfsq - (s * (hfsq + R) + dk * 1.90821492927058770002e-10)) - f);
}
#ifndef QPD_MC_PAIRS
#define QPD_MC_PAIRS 1  // noise pairs per lane and round: 1 measured best (2: +1 %, 4: +5 % generator time; profiles/r03n_ab_generator_pairs.txt)
#endif
#ifndef QPD_MC_WPE
#define QPD_MC_WPE 6  // 6 waves per SIMD: -2.5 % generator time vs 5 (profiles/r03j_ab_generator.txt)
#endif

// The encoder on one frame's bit words (one wave, lane t; bw written and a
// barrier passed): u word w = the info bits [pref_w, pref_w + popc(mask_w))
// deposited at the mask's set bits, one 16-bit half per lane (the deposit loop
// runs popc(half) <= 16 times); then the 5 in-word stages of x = u F^{(x)n}
// (bit i ^= bit i + m for i with bit m clear) and the word stages in LDS.  Ends
// with a barrier: xw[0 .. nw) is the codeword.
__device__ __forceinline__ void mc_encode_words(const McChannel &C, int t, int nw, const uint32_t *bw, uint32_t *xw) {
    for (int h0 = 0; h0 < 2 * nw; h0 += 64) {  // whole-wave rounds: the halves meet by a shuffle
        const int h = h0 + t, w = h >> 1;
        uint32_t u = 0;
        if (h < 2 * nw) {
            const uint32_t wm = C.info_mask[w];
            uint32_t mask = (h & 1) ? wm >> 16 : wm & 0xFFFFu;
            const int s = C.info_pref[w] + ((h & 1) ? __builtin_popcount(wm & 0xFFFFu) : 0);
            const uint32_t lo = bw[s >> 5], hi = bw[(s >> 5) + 1];
            uint32_t src = (s & 31) ? ((lo >> (s & 31)) | (hi << (32 - (s & 31)))) : lo;
            for (; mask; mask &= mask - 1u) {
                u |= (src & 1u) << __builtin_ctz(mask);
                src >>= 1;
            }
        }
        u |= (uint32_t)__shfl_xor((int)u, 1, 64) << 16;  // even lane: low | high << 16
        if (h < 2 * nw && !(h & 1)) {
            u ^= (u >> 1) & 0x55555555u;
            u ^= (u >> 2) & 0x33333333u;
            u ^= (u >> 4) & 0x0F0F0F0Fu;
            u ^= (u >> 8) & 0x00FF00FFu;
            u ^= (u >> 16) & 0x0000FFFFu;
            xw[w] = u;
        }
    }
    __syncthreads();
    for (int sw = 1; sw < nw; sw <<= 1) {  // word stages (m = 32 sw)
        for (int w = t; w < nw; w += 64)
            if (!(w & sw)) xw[w] ^= xw[w + sw];
        __syncthreads();
    }
}

// The two Gaussians of positions 2p and 2p+1 of frame (glo, ghi): one Philox
// block, Box-Muller on its two 52-bit uniforms.
__device__ __forceinline__ void mc_noise_pair(const McChannel &C, uint32_t glo, uint32_t ghi, int p, double (&nz)[2]) {
    const Philox4 r = philox4x32_10(glo, ghi, (uint32_t)p, kTagNoise, C.seed_lo, C.seed_hi);
    const double u1 = 2.0 - mc_one_m(r.v[0], r.v[1]);  // (0, 1]
    const double u2 = mc_one_m(r.v[2], r.v[3]) - 1.0;  // [0, 1)
    const double rad = sqrt(-2.0 * mc_log(u1));
    double sn, cs;
    mc_sincos(6.283185307179586 * u2, &sn, &cs);
    nz[0] = rad * cs;
    nz[1] = rad * sn;
}

// One position: y = bpsk(xbit) + sigma nz (no_signal: sigma nz alone, an empty
// candidate), llr = y * 2 * inv_s2, without fused multiply-adds; returned.  QUANT:
// *s_out = the driver's channel symbol of llr, from the staged tables E (E[0] =
// -inf, E[1 + i] = edges[i]) and lut: bisect_left over edges[0..M-1] for
// lo_edge < llr < hi_edge gives lo in [1, M] with edges[lo - 1] < llr <= edges[lo];
// guessed, checked, walked if wrong.
template <bool QUANT>
__device__ __forceinline__ double mc_llr_symbol(const McChannel &C, uint32_t xbit, bool no_signal, double nzh,
                                                const double *E, const int32_t *lut, double lo_edge, double hi_edge,
                                                double inv_w, int M, int *s_out) {
#pragma clang fp contract(off)
    const double bpsk = xbit ? -1.0 : 1.0;
    const double sn = C.sigma * nzh;
    const double y = no_signal ? sn : bpsk + sn;
    const double llr = y * 2.0 * C.inv_s2;
    if constexpr (QUANT) {
        const bool inner = llr > lo_edge && llr < hi_edge;
        const double gi = fmin(fmax((llr - lo_edge) * inv_w + 1.0, 1.0), (double)M);
        int lo = (int)gi;
        if (inner && !(E[lo] < llr && llr <= E[lo + 1])) {
            while (E[lo] >= llr) --lo;     // stops at lo >= 1: E[1] = lo_edge < llr
            while (E[lo + 1] < llr) ++lo;  // stops at lo <= M: E[M + 1] = hi_edge > llr
        }
        const int sl = lut[lo - 1];
        *s_out = inner ? sl : (llr <= lo_edge ? 0 : C.q - 1);
    }
    return llr;
}

}  // namespace qpd
