// qpd_fast_pre.hpp -- the fast engine's root pre-pass kernel (pre-mode), launched
// by qpd_capi.hip before the decode kernels of qpd_fast.hip, and the widening copy
// of uint8 channel symbols for the decoders that have no pre-pass (widen_u8_kernel).
#pragma once
#include "qpd_fast_switches.hpp"

#include "qpd_fast_lookup.hpp"

namespace qpd {

// ---------------------------------------------------------------------------
// Root pre-pass (pre-mode: N >= 16, the root's left child a plain node).
// The root's f and both g variants depend on the channel symbols only, yet
// every path of a frame computes them (SCLLUTDecoder.cpp:83-89 / :157-164 at
// depth 0: L x N lookups per frame), and the decode kernel would read the
// frame's 4 KB of int32 symbols twice, half a decode apart.  Here one thread
// per output word computes them once per frame from one coalesced read of the
// channel, into a row of N/4 words per frame: [f(y) | g(y, 0) | g(y, 1) | -],
// N/16 words each, 8 nibble symbols per word as S[1].  The decode kernel then
// reads the left child's S[1] from the row (MF_PRE) and builds the root g by
// nibble selects (MF_GSEL, gsel_op).  Out-of-range symbols raise the error
// flag here, as chan_word8 does in the decode kernel.
// ---------------------------------------------------------------------------
// The root's f and g tables as bytes in LDS once per block (stage_tab): an
// element's 8-bit index addresses all three results (f, g with u = 0 at +0,
// u = 1 at +256) -- one field extract and three ds_read_u8 per element.
// LO (rows in lookup order, QPD_ROW_BYTEIDX: FastHostPlan::row_lo): each of the three
// rows as S[1] in that order -- word w holds child elements 4w .. 4w+3 in the high
// nibbles and N/4 + 4w .. in the low ones, so the thread of word w reads the channel's
// four runs of four symbols at 4w, N/4 + 4w, N/2 + 4w, 3N/4 + 4w: the same lookups and
// bytes, one store per row as before.
template <class In, bool LO = false>
__global__ __launch_bounds__(256) void root_pre_kernel(FastPlan P, const In *__restrict__ in, int64_t B,
                                                       uint32_t *__restrict__ pre) {
    __shared__ __attribute__((aligned(16))) uint8_t tf[256], tg[512];
    if (threadIdx.x < 64) {  // node 0 (posi 0)
        stage_tab(tg, P.g_tab[threadIdx.x], threadIdx.x);
        if (threadIdx.x < 32) stage_tab(tf, P.f_tab[threadIdx.x], threadIdx.x);
    }
    __syncthreads();
    const int wsh = P.n - 4;  // log2 words per segment
    const int half = P.N >> 1;
    const int64_t total = B << wsh;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < total; base += (int64_t)gridDim.x * 256) {
        const int64_t t0 = base + threadIdx.x;
        const int64_t t = t0 < total ? t0 : total - 1;
        const int64_t f = t >> wsh;
        const int w = (int)(t & ((1 << wsh) - 1));
        const In *y = in + (f << P.n);
        const int quarter = P.N >> 2;
        const uint32_t a = LO ? chan_word44(y, 4 * w, quarter + 4 * w, P.in_vec, P.v, P.err) : chan_word8(y, 8 * w, P.in_vec, P.v, P.err);
        const uint32_t b = LO ? chan_word44(y, half + 4 * w, half + quarter + 4 * w, P.in_vec, P.v, P.err)
                              : chan_word8(y, half + 8 * w, P.in_vec, P.v, P.err);
        const uint32_t X = ((a << 4) & 0xF0F0F0F0u) | (b & 0x0F0F0F0Fu);  // byte j: index of element 2j
        const uint32_t Y = (a & 0xF0F0F0F0u) | ((b >> 4) & 0x0F0F0F0Fu);  // ... of element 2j + 1
        uint32_t fw = 0, g0 = 0, g1 = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t idx = __builtin_amdgcn_ubfe((k & 1) ? Y : X, 8 * (k >> 1), 8);
            const int at = 4 * (LO ? il_nib<8>(k) : k);  // (LO: lookup k is child element 4w + k / N/4 + 4w + k - 4)
            fw |= (uint32_t)tf[idx] << at;
            g0 |= (uint32_t)tg[idx] << at;
            g1 |= (uint32_t)tg[256 + idx] << at;
        }
        if (t0 < total) {
            uint32_t *row = pre + (f << (P.n - 2));
            row[w] = fw;
            row[(1 << wsh) + w] = g0;
            row[(2 << wsh) + w] = g1;
        }
    }
}

// ---------------------------------------------------------------------------
// uint8 channel symbols of everything that is not pre-mode (the generic engine;
// fast-engine decoders of N < 16, with a special left child of the root or under
// QPD_NO_PRE): widened into a handle-owned int32 staging buffer, chunk by chunk,
// for the int32 launch that exists (qpd_capi.hip: decode_u8_impl).  None of
// these is a hot path -- the generic engine decodes 0.4-0.6 M frames/s, frames
// of N < 16 are a few bytes -- so their kernels are not templates over the
// input type: one more copy of each would buy nothing measurable.  The range
// check stays in the int32 readers.  Four symbols per thread (one 32-bit load,
// one 128-bit store) where the source is 4-byte aligned, else one.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void widen_u8_kernel(const uint8_t *__restrict__ in, int64_t n,
                                                       int32_t *__restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t done = 0;
    if (((uintptr_t)in & 3u) == 0) {
        const int64_t nq = n >> 2;
        for (int64_t q = t; q < nq; q += stride) {
            const uint32_t x = ((const uint32_t *)in)[q];
            ((int4 *)out)[q] = make_int4((int)(x & 255u), (int)((x >> 8) & 255u), (int)((x >> 16) & 255u), (int)(x >> 24));
        }
        done = nq << 2;
    }
    for (int64_t i = done + t; i < n; i += stride) out[i] = in[i];
}

}  // namespace qpd
