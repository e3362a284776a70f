// qpd_fast_lookup.hpp -- the fast engine's table lookups and the ops made of them
// alone: the re-encode's word steps, the pointer fields, the channel readers,
// lut_vec / lut_byte / lut_lds, the f / g ops (fg_op, fg_chan_op, ff_op, gsel_op) and the
// per-op operand prefetch (fetch_pre).
#pragma once
#include "qpd_fast_switches.hpp"

#include "qpd_fast_plan.hpp"

namespace qpd {

__device__ __forceinline__ uint32_t bperm(uint32_t table, uint32_t dword) {
    return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(dword << 2), (int)table);
}

// 4-bit LUT lookup from the table register: entry idx lives in dword idx>>3.
__device__ __forceinline__ uint32_t lut4(uint32_t table, uint32_t idx) {
    return (bperm(table, idx >> 3) >> ((idx & 7u) << 2)) & 15u;
}

// x F^{(x)5} inside one 32-bit word (the in-word stages of the re-encode).
__device__ __forceinline__ uint32_t polar_word(uint32_t x) {
    x ^= (x >> 1) & 0x55555555u;
    x ^= (x >> 2) & 0x33333333u;
    x ^= (x >> 4) & 0x0f0f0f0fu;
    x ^= (x >> 8) & 0x00ff00ffu;
    x ^= (x >> 16) & 0x0000ffffu;
    return x;
}

// Cross-word butterfly stage of the re-encode on a register row (nwr <= 32 words).
template <int MW>
__device__ __forceinline__ void xor_stage(uint32_t (&x)[32], int nwr) {
#pragma unroll
    for (int i = 0; i < 32; i += 2 * MW)
#pragma unroll
        for (int j = 0; j < MW; ++j)
            if (i + MW + j < nwr) x[i + j] ^= x[i + MW + j];
}

__device__ __forceinline__ int pfield(uint64_t p, int sh) { return (int)((p >> sh) & 15u); }
__device__ __forceinline__ uint64_t pset(uint64_t p, int sh, int gl) {
    return (p & ~(15ull << sh)) | ((uint64_t)gl << sh);
}

// Channel symbols: int32 input, range-checked (UB in the reference).
__device__ __forceinline__ uint32_t chan_sym(const int32_t *y, int e, int v, int32_t *err) {
    int s = y[e];
    if ((unsigned)s >= (unsigned)v) {
        atomicOr(err, 1);
        s = 0;
    }
    return (uint32_t)s;
}

__device__ __forceinline__ uint32_t chan_word(const int32_t *y, int e0, int cnt, int v, int32_t *err) {
    uint32_t w = 0;
    for (int i = 0; i < cnt; ++i) w |= chan_sym(y, e0 + i, v, err) << (4 * i);
    return w;
}

// Eight channel symbols e0..e0+7 as one nibble word; `vec` = the input rows
// are 16-byte aligned (two 128-bit loads instead of eight 32-bit ones).
__device__ __forceinline__ uint32_t chan_word8(const int32_t *y, int e0, bool vec, int v, int32_t *err) {
    if (!vec) return chan_word(y, e0, 8, v, err);
    const int4 a = *(const int4 *)(y + e0), b = *(const int4 *)(y + e0 + 4);
    const int e[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t w = 0, bad = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t s = (uint32_t)e[i];
        bad |= s >= (uint32_t)v;
        w |= (s >= (uint32_t)v ? 0u : s) << (4 * i);
    }
    if (bad) atomicOr(err, 1);
    return w;
}

// Channel symbols e0..e0+3 (nibbles 0-3) and e1..e1+3 (nibbles 4-7), e0 and e1 multiples
// of 4: the two runs of a word of a row in lookup order (QPD_ROW_BYTEIDX).
__device__ __forceinline__ uint32_t chan_word44(const int32_t *y, int e0, int e1, bool vec, int v, int32_t *err) {
    if (!vec) return chan_word(y, e0, 4, v, err) | (chan_word(y, e1, 4, v, err) << 16);
    const int4 a = *(const int4 *)(y + e0), b = *(const int4 *)(y + e1);
    const int e[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t w = 0, bad = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t s = (uint32_t)e[i];
        bad |= s >= (uint32_t)v;
        w |= (s >= (uint32_t)v ? 0u : s) << (4 * i);
    }
    if (bad) atomicOr(err, 1);
    return w;
}

// The same from uint8 input (qpd_decode_u8; read by root_pre_kernel only, so v <= 16).
// `vec` = the input rows are 8-byte aligned: the eight symbols are one 64-bit
// load, range-checked and packed SWAR.  A byte is out of range when its high
// nibble is set or its low nibble is >= v: adding 16 - v to the low nibbles
// carries into bit 4 exactly then (at most 15 + 14: no carry leaves the byte).
// As for int32, a bad symbol decodes as 0 and raises the error word.
__device__ __forceinline__ uint32_t chan_word(const uint8_t *y, int e0, int cnt, int v, int32_t *err) {
    uint32_t w = 0, bad = 0;
#pragma unroll 1
    for (int i = 0; i < cnt; ++i) {
        const uint32_t s = y[e0 + i];
        bad |= s >= (uint32_t)v;
        w |= (s >= (uint32_t)v ? 0u : s) << (4 * i);
    }
    if (bad) atomicOr(err, 1);
    return w;
}

__device__ __forceinline__ uint32_t nib_pack4(uint32_t x) {  // bytes 0-3 of x (each < 16) -> nibbles 0-3
    const uint32_t t = (x | (x >> 4)) & 0x00FF00FFu;
    return (t | (t >> 8)) & 0xFFFFu;
}

// Eight symbols as the bytes of x: range-checked and packed SWAR (see above).
__device__ __forceinline__ uint32_t chan_pack8(uint2 x, int v, int32_t *err) {
    const uint32_t k = (uint32_t)(16 - v) * 0x01010101u;
    uint32_t lo0 = x.x & 0x0F0F0F0Fu, lo1 = x.y & 0x0F0F0F0Fu;
    // bits 7:4 of each byte: the high nibble, or the carry of low nibble + 16 - v
    const uint32_t t0 = (x.x & 0xF0F0F0F0u) | ((lo0 + k) & 0x10101010u);
    const uint32_t t1 = (x.y & 0xF0F0F0F0u) | ((lo1 + k) & 0x10101010u);
    if (t0 | t1) {  // rare: clear the bad bytes (nibble != 0 -> bit 4 -> 0x0F)
        const uint32_t f0 = (((t0 >> 4) & 0x0F0F0F0Fu) + 0x0F0F0F0Fu) & 0x10101010u;
        const uint32_t f1 = (((t1 >> 4) & 0x0F0F0F0Fu) + 0x0F0F0F0Fu) & 0x10101010u;
        lo0 &= ~(f0 - (f0 >> 4));
        lo1 &= ~(f1 - (f1 >> 4));
        atomicOr(err, 1);
    }
    return nib_pack4(lo0) | (nib_pack4(lo1) << 16);
}

__device__ __forceinline__ uint32_t chan_word8(const uint8_t *y, int e0, bool vec, int v, int32_t *err) {
    if (!vec) return chan_word(y, e0, 8, v, err);
    return chan_pack8(*(const uint2 *)(y + e0), v, err);
}

__device__ __forceinline__ uint32_t chan_word44(const uint8_t *y, int e0, int e1, bool vec, int v, int32_t *err) {
    if (!vec) return chan_word(y, e0, 4, v, err) | (chan_word(y, e1, 4, v, err) << 16);
    return chan_pack8(make_uint2(*(const uint32_t *)(y + e0), *(const uint32_t *)(y + e1)), v, err);
}

// Word w (8 symbols) of S[d] of the path whose slot is `src`.
// The first `cnt` channel symbols as one nibble word, a rolled loop: the
// channel reads of the ops that see the channel only in codes of N <= 8 (the
// BOT3 / leaf ops at the root) -- small code for a case that is never hot.
__device__ __forceinline__ uint32_t chan_small(const int32_t *y, int cnt, int v, int32_t *err) {
    uint32_t w = 0, bad = 0;
#pragma unroll 1
    for (int i = 0; i < cnt; ++i) {
        const uint32_t s = (uint32_t)y[i];
        bad |= s >= (uint32_t)v;
        w |= (s >= (uint32_t)v ? 0u : s) << (4 * i);
    }
    if (bad) atomicOr(err, 1);
    return w;
}

// Word w of S[d]: the pre-pass row (MF_PRE), a slab / LDS row, or with CH the
// channel (MF_CHAN): the ops that read the channel only in codes of N <= 8
// (the BOT3 / leaf ops at the root; word 0, chan_small).  The f / g ops at
// the root read it in fg_chan_op.
template <bool CH = false>
__device__ __forceinline__ uint32_t sym_word(const FastPlan &P, const Mem &M, const MOp &op, const int32_t *y, int src,
                                             int w, int cnt = 8) {
    if (op.flags & MF_PRE) return ((const uint32_t *)y)[op.src_row + w];  // N >= 16: whole words
    if constexpr (CH)
        if (op.flags & MF_CHAN) return chan_small(y, cnt, P.v, P.err);
    return M.ld(op.flags & MF_SRC_LDS, op.src_row + w, src);
}

// NE table lookups T[a_i, b_i] (i < NE <= 8) packed as output nibbles, with
// a_i / b_i = nibble i of A / B and table half h_i = bit i of `hi` (the g
// table's u = 1 half, or the second of two packed f tables).  SWAR index
// build: byte j of X / Y is the 8-bit index of element 2j / 2j+1, from which
// one pass each derives the ds_bpermute byte address (idx >> 1, whose bits
// 7:2 select the dword; + 128 for the upper half) and the nibble offset
// ((idx & 7) * 4, used by v_bfe through its low 5 bits only).
// IL (NE = 8, both producers): the results in interleaved order for lut_byte
// below -- element k at nibble il_nib<8>(k) -- instead of element k at nibble k.
template <int NE>
__device__ constexpr int il_nib(int k) { return k < NE / 2 ? 2 * k + 1 : 2 * (k - NE / 2); }

// Bit k of c (c < 16) -> bit 8k: one 24-bit multiply (full rate) copies c to distances
// 7, 14, 21; no two copies' bits meet, so nothing carries.
__device__ __forceinline__ uint32_t byte_bits4(uint32_t c) { return __umul24(c, 0x204081u) & 0x01010101u; }

// LO (NE = 8; rows in lookup order, QPD_ROW_BYTEIDX): A and B are two words of a row
// in that order, so their bytes are the eight indices as they lie -- element k < 4 is
// byte k of A, element k >= 4 byte k - 4 of B, table half bit k of `hi` as ever -- and
// no X / Y is built.  With IL the result is the child row's word in lookup order.
template <int NE, bool IL = false, bool LO = false>
__device__ __forceinline__ uint32_t lut_vec(uint32_t T, uint32_t A, uint32_t B, uint32_t hi, uint32_t hi2 = 0u) {
    static_assert(!LO || NE == 8, "LO: whole words of a row in lookup order");
    if constexpr (LO) {  // (table halves: bits 0-3 of hi for A's elements, of hi2 for B's)
        const uint32_t ha = byte_bits4(hi & 15u) << 7, hb = byte_bits4(hi2 & 15u) << 7;
        const uint32_t AA = ((A >> 1) & 0x7F7F7F7Fu) | ha, BA = ((B >> 1) & 0x7F7F7F7Fu) | hb;
        const uint32_t AS = (A << 2) & 0x1C1C1C1Cu, BS = (B << 2) & 0x1C1C1C1Cu;
        uint32_t out = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int j = k & 3;
            const uint32_t WA = k < 4 ? AA : BA, WS = k < 4 ? AS : BS;
            const uint32_t v = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(WA >> (8 * j)), (int)T);
            out |= __builtin_amdgcn_ubfe(v, WS >> (8 * j), 4) << (4 * (IL ? il_nib<NE>(k) : k));
#if QPD_VEC_CHAIN
            if (k + 1 < NE) asm("" : "+v"(out));
#endif
        }
        return out;
    }
    const uint32_t X = ((A << 4) & 0xF0F0F0F0u) | (B & 0x0F0F0F0Fu);
    const uint32_t Y = (A & 0xF0F0F0F0u) | ((B >> 4) & 0x0F0F0F0Fu);
    uint32_t hx = 0, hy = 0;  // bit 2j / 2j+1 of hi -> bit 8j+7
    if constexpr (NE == 8) {  // one multiply spreads 4 bits (no carries reach the kept bits)
        hx = ((hi & 0x55u) * 0x02082080u) & 0x80808080u;
        hy = (((hi >> 1) & 0x55u) * 0x02082080u) & 0x80808080u;
    } else {
#pragma unroll
        for (int j = 0; 2 * j < NE; ++j) {
            hx |= ((hi >> (2 * j)) & 1u) << (8 * j + 7);
            hy |= ((hi >> (2 * j + 1)) & 1u) << (8 * j + 7);
        }
    }
    const uint32_t XA = ((X >> 1) & 0x7F7F7F7Fu) | hx;
    const uint32_t YA = ((Y >> 1) & 0x7F7F7F7Fu) | hy;
    const uint32_t XS = (X << 2) & 0x1C1C1C1Cu, YS = (Y << 2) & 0x1C1C1C1Cu;
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        const int j = k >> 1;
        const uint32_t WA = (k & 1) ? YA : XA, WS = (k & 1) ? YS : XS;
        // ds_bpermute reads lane (addr >> 2) & 63: the bytes above j need no mask
        const uint32_t v = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(WA >> (8 * j)), (int)T);
        out |= __builtin_amdgcn_ubfe(v, WS >> (8 * j), 4) << (4 * (IL ? il_nib<NE>(k) : k));
#if QPD_VEC_CHAIN
        if (k + 1 < NE) asm("" : "+v"(out));  // one v_lshl_or per element, not shifts + v_or3
#endif
    }
    return out;
}

// Interleaved order: a word of NE = 2 / 4 / 8 symbols whose element k (k < NE / 2)
// sits in the high nibble of byte k and element k + NE / 2 in the low nibble.
// Byte k is then the table index a * 16 + b of the f / g lookup of elements
// (k, k + NE / 2) as it lies.  nib_interleave8: a word in element order
// (nibble i = element i) into that order, one v_perm and a nibble swap.
__device__ __forceinline__ uint32_t nib_interleave8(uint32_t w) {
    const uint32_t t = __builtin_amdgcn_perm(w, w, 0x01030002u);  // bytes [e4 e5 | e0 e1 | e6 e7 | e2 e3]
    return (t & 0xF00FF00Fu) | ((t & 0x00F000F0u) << 4) | ((t >> 4) & 0x00F000F0u);
}

// Bit k of c -> bit 8k + 7: the table halves of lut_byte's elements from two (c < 4)
// or four (c < 16) u bits.  One 24-bit multiply (full rate) copies c to distances
// 7, 14 (, 21, 28 after the shift); no two copies' bits meet, so nothing carries.
__device__ __forceinline__ uint32_t half_bits2(uint32_t c) { return __umul24(c, 0x4080u) & 0x8080u; }
__device__ __forceinline__ uint32_t half_bits4(uint32_t c) {
    uint32_t m = __umul24(c, 0x204081u);
    asm("" : "+v"(m));  // else the shift is folded into a 32-bit multiply (v_mul_lo_u32: quarter rate)
    return (m << 7) & 0x80808080u;
}

// NE = 2 or 4 lookups T[byte k of W] (QPD_BOT3_BYTEIDX: BOT3's internal nodes),
// W in interleaved order: no index build.  The ds_bpermute address of element k
// is bits 8k+1 .. 8k+7 (the low two address bits are ignored), with H (HAS_H: bit
// 8k + 7 = the table half of element k -- the g table's u = 1 half, or the second
// of two packed f tables) put above the index once for the word; the nibble
// offset is (byte & 7) * 4, masked once for the word (v_bfe reads its low five
// bits).  IL: the results in interleaved order again (NE = 4: W2 from W3), else
// element k at nibble k (NE = 2: the leaf pair's W1 as leaf_idx reads it).
// Bits of W above byte NE - 1 are ignored.
template <int NE, bool IL, bool HAS_H>
__device__ __forceinline__ uint32_t lut_byte(uint32_t T, uint32_t W, uint32_t H = 0u) {
    constexpr uint32_t M7 = NE == 4 ? 0x7F7F7F7Fu : 0x7F7Fu, M3 = NE == 4 ? 0x1C1C1C1Cu : 0x1C1Cu;
    const uint32_t WS = (W << 2) & M3;
    uint32_t WA = 0;
    if constexpr (HAS_H) WA = ((W >> 1) & M7) | (H & ~M7);
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        // (HAS_H: ds_bpermute reads lane (addr >> 2) & 63, the bytes above k need no mask)
        const uint32_t addr = HAS_H ? WA >> (8 * k) : __builtin_amdgcn_ubfe(W, 8 * k + 1, 7);
        const uint32_t v = (uint32_t)__builtin_amdgcn_ds_bpermute((int)addr, (int)T);
        out |= __builtin_amdgcn_ubfe(v, WS >> (8 * k), 4) << (4 * (IL ? il_nib<NE>(k) : k));
    }
    return out;
}

// The same NE lookups from the op's table staged as bytes in LDS (SCL-LUT's
// f / g ops: stage_tab, then lut_lds): entry i of the f table (256) or of the
// g table (512: u = 0, then u = 1) at byte i, read by ds_read_u8.  The address
// of element k is byte j = k/2 of X / Y (one v_bfe; for g, v_perm_b32 puts the
// u bit above it), and the result is the nibble itself: two VALU per lookup
// against about five for the bpermute form, whose address and nibble offset
// need a shift each and the result a field extract.  The f table's 64 dwords
// sit one per LDS bank (conflict-free); the g table's two halves share banks.
__device__ __forceinline__ uint32_t nib2byte4(uint32_t x) {  // nibbles 0-3 of x -> bytes 0-3
    x = (x | (x << 8)) & 0x00FF00FFu;
    return (x | (x << 4)) & 0x0F0F0F0Fu;
}

// Table dword `dw` (8 entries: f lanes & 31, g all 64 lanes) as 8 bytes at tb + 8 * dw.
__device__ __forceinline__ void stage_tab(uint8_t *tb, uint32_t T, int dw) {
    uint2 b;
    b.x = nib2byte4(T & 0xFFFFu);
    b.y = nib2byte4(T >> 16);
    *(uint2 *)(tb + 8 * dw) = b;
}

// Bank swizzle of the g table's u = 1 half (QPD_GSWZ, qpd_fast_switches.hpp; off).
__device__ __forceinline__ int gtab_dw(int lane) { return lane ^ ((lane >> 5) * (QPD_GSWZ >> 3)); }

// The staged tables sit at LDS offset TOFF of the wave's allocation (the kernel's
// `tb`, offset 0: lut_fast_kernel puts them first; qpd_capi.hip checks that the
// kernel declares no static LDS before them): the lookups address LDS through a
// constant, which the compiler folds into each ds_read_u8's offset field.
typedef __attribute__((address_space(3))) const uint8_t lds_u8;
// LO (NE = 8; as lut_vec): A / B are the index words of elements 0-3 / 4-7 as they
// lie in a row in lookup order, bits 0-3 of `hi` / of `hi2` their table halves.
template <int NE, bool ISG, int TOFF = 0, bool IL = false, bool LO = false>
__device__ __forceinline__ uint32_t lut_lds(uint32_t A, uint32_t B, uint32_t hi, uint32_t hi2 = 0u) {
    static_assert(!LO || (NE == 8 && QPD_GSWZ == 0), "LO: whole words of a row in lookup order");
    lds_u8 *const tb = (lds_u8 *)(size_t)TOFF;
    uint32_t X = LO ? A : ((A << 4) & 0xF0F0F0F0u) | (B & 0x0F0F0F0Fu);
    uint32_t Y = LO ? B : (A & 0xF0F0F0F0u) | ((B >> 4) & 0x0F0F0F0Fu);
    uint32_t hx = 0, hy = 0;  // byte j = bit 2j / 2j+1 of hi (g: the u half); LO: bit j of hi / hi2
    if constexpr (ISG && LO) {
        hx = byte_bits4(hi & 15u);
        hy = byte_bits4(hi2 & 15u);
    } else if constexpr (ISG) {
        hx = (((hi & 0x55u) * 0x02082080u) >> 7) & 0x01010101u;
        hy = ((((hi >> 1) & 0x55u) * 0x02082080u) >> 7) & 0x01010101u;
        if constexpr (QPD_GSWZ != 0) {  // bytes of hx, hy are 0 / 1: X ^= hx * M by shifts (a
            uint32_t sx = 0, sy = 0;      // 32-bit multiply is a quarter-rate VALU op)
#pragma unroll
            for (int bit = 3; bit < 8; ++bit)
                if ((QPD_GSWZ >> bit) & 1) {
                    sx |= hx << bit;
                    sy |= hy << bit;
                }
            X ^= sx;
            Y ^= sy;
        }
    }
#if QPD_LUT_OPAQUE_XY
    // the words whole: otherwise the compiler rebuilds each index's byte from A and B
    // (v_and + v_bitop3 chains) beside X / Y themselves -- 15 VALU for 8 f indices, not 12
    if constexpr (!LO) asm("" : "+v"(X), "+v"(Y));
#endif
    uint32_t idx[NE];
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        const int j = LO ? (k & 3) : (k >> 1);
        const bool second = LO ? k >= 4 : (k & 1) != 0;
        const uint32_t W = second ? Y : X;
        if constexpr (ISG)  // byte 0 = byte j of W, byte 1 = byte j of the u bits, bytes 2-3 = 0
            idx[k] = __builtin_amdgcn_perm(second ? hy : hx, W, (uint32_t)(j | ((4 + j) << 8) | (0x0C << 16) | (0x0C << 24)));
        else
            idx[k] = __builtin_amdgcn_ubfe(W, 8 * j, 8);
#if QPD_EXP_LUTMASK != 0xFFFF
        idx[k] &= QPD_EXP_LUTMASK;
#endif
    }
#if QPD_LUT_PACK2
    if constexpr (NE == 8) {
        // The even elements' bytes as [e0, e2, e4, e6] (16-bit pairs: the compiler
        // joins two loaded bytes with one v_perm), the odd ones' likewise, then one
        // shift-or: 7 VALU for the 8 results (4 v_perm, 3 v_lshl_or) instead of a
        // shift per element and an or3 per two.  O passes through an empty asm so
        // that the compiler does not distribute the final shift over O's two
        // halves (v_lshlrev x2 + v_or3 instead of one v_lshl_or: +1 VALU per word).
        // IL (interleaved order, see lut_byte): the low nibbles are elements 4-7, the
        // high ones elements 0-3 -- only which loaded bytes are paired changes.
        typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
        constexpr int e0 = IL ? 4 : 0, e1 = IL ? 6 : 4, e2 = IL ? 5 : 2, e3 = IL ? 7 : 6;
        constexpr int o0 = IL ? 0 : 1, o1 = IL ? 2 : 5, o2 = IL ? 1 : 3, o3 = IL ? 3 : 7;
        const u16x2 r0 = {tb[idx[e0]], tb[idx[e1]]}, r1 = {tb[idx[e2]], tb[idx[e3]]};
        const u16x2 s0 = {tb[idx[o0]], tb[idx[o1]]}, s1 = {tb[idx[o2]], tb[idx[o3]]};
        const uint32_t E = __builtin_bit_cast(uint32_t, r0) | (__builtin_bit_cast(uint32_t, r1) << 8);
        uint32_t O = __builtin_bit_cast(uint32_t, s0) | (__builtin_bit_cast(uint32_t, s1) << 8);
#if QPD_LUT_OPAQUE
        asm("" : "+v"(O));
#endif
        return E | (O << 4);
    }
#endif
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < NE; ++k) out |= (uint32_t)tb[idx[k]] << (4 * (IL ? il_nib<NE>(k) : k));
    return out;
}

// f / g op (SCLLUTDecoder.cpp:83-89 / :157-164): child symbols at depth d+1,
// for each of the wave's NS frame sets.  Words are processed in chunks whose
// loads are all issued before the first lookup: the shallow levels live in
// the global slab, and one memory round trip per chunk instead of per word is
// what bounds these ops.
// Source word of an f/g op; RAW: S[d] is a slab/LDS row (no channel / pre-pass
// reads), decided once per op instead of per word.
// SL >= 0: the row space of S[d] fixed at compile time (0 slab, 1 LDS).
template <bool RAW, int SL = -1>
__device__ __forceinline__ uint32_t fg_word(const FastPlan &P, const Mem &M, const MOp &op, const int32_t *y, int src, int w,
                                            int cnt = 8) {
    if constexpr (RAW) return M.ld(SL >= 0 ? SL != 0 : (op.flags & MF_SRC_LDS) != 0, op.src_row + w, src);
    return sym_word(P, M, op, y, src, w, cnt);
}

// f / g op at the root on the channel symbols (MF_CHAN: codes without the
// root pre-pass), a rolled loop over its words -- one copy of the channel
// reads (range check, error flag) instead of one per unrolled word.
// LO: S[1] is written in lookup order -- word w from the channel's four runs of four
// symbols at 4w, 4 (nwo + w), 4 (2 nwo + w), 4 (3 nwo + w).
template <bool ISG, int NS, bool LO = false>
__device__ __forceinline__ void fg_chan_op(const FastPlan &P, const Mem (&M)[NS], const MOp &op, const int32_t *const (&y)[NS],
                                           const int (&usrc)[NS], uint32_t T, int lane) {
    const int ctemp = op.cnt;
    const bool dl = op.flags & MF_DST_LDS, ul = op.flags & MF_U_LDS;
    if (LO && ctemp >= 8) {
        const int nwo = ctemp >> 3;
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll 1
            for (int w = 0; w < nwo; ++w) {
                const uint32_t a = chan_word(y[s], 4 * w, 4, P.v, P.err) | (chan_word(y[s], 4 * (nwo + w), 4, P.v, P.err) << 16);
                const uint32_t b = chan_word(y[s], 4 * (2 * nwo + w), 4, P.v, P.err) |
                                   (chan_word(y[s], 4 * (3 * nwo + w), 4, P.v, P.err) << 16);
                uint32_t ub = 0u;
                if (ISG) {
                    const int ba = 4 * w, bb = 4 * (nwo + w);  // u bits of the word's high- / low-nibble elements
                    ub = ((M[s].ld(ul, op.u_row + (ba >> 5), usrc[s]) >> (ba & 31)) & 15u) |
                         (((M[s].ld(ul, op.u_row + (bb >> 5), usrc[s]) >> (bb & 31)) & 15u) << 4);
                }
                M[s].st(dl, op.dst_row + w, lane, lut_vec<8, true>(T, a, b, ub));
            }
    } else if (ctemp >= 8) {
        const int nwo = ctemp >> 3;
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll 1
            for (int w = 0; w < nwo; ++w) {
                const uint32_t a = chan_word8(y[s], 8 * w, P.in_vec, P.v, P.err);
                const uint32_t b = chan_word8(y[s], 8 * (nwo + w), P.in_vec, P.v, P.err);
                const uint32_t ub = ISG ? M[s].ld(ul, op.u_row + (w >> 2), usrc[s]) >> ((w & 3) << 3) : 0u;
                M[s].st(dl, op.dst_row + w, lane, lut_vec<8>(T, a, b, ub));
            }
    } else {  // ctemp in {2, 4}: the whole root (a then b) in one word
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const uint32_t W = chan_small(y[s], 2 * ctemp, P.v, P.err);
            const uint32_t ub = ISG ? M[s].ld(ul, op.u_row, usrc[s]) : 0u;
            const uint32_t out = ctemp == 4 ? lut_vec<4>(T, W, W >> 16, ub) : lut_vec<2>(T, W, W >> 8, ub);
            M[s].st(dl, op.dst_row, lane, out);
        }
    }
}

// LT: lookups from the byte table staged at tb (lut_lds) instead of T.
// LO (rows in lookup order, QPD_ROW_BYTEIDX): S[d] and S[d+1] (>= 8 symbols each) are in
// that order; the same word pairs (w, nwo + w) are read, as index words, and the u bits of
// output word w are bits 4w .. 4w+3 and 4 (nwo + w) .. of U[d+1].
template <bool ISG, bool RAW, int NS, int SL = -1, int DL = -1, bool LT = false, bool LO = false>
__device__ __forceinline__ void fg_op(const FastPlan &P, const Mem (&M)[NS], const MOp &op, const int32_t *const (&y)[NS],
                                      const int (&src)[NS], const int (&usrc)[NS], uint32_t T, int lane,
                                      const uint8_t *tb = nullptr) {
    const int ctemp = op.cnt;
    const bool dl = DL >= 0 ? DL != 0 : (op.flags & MF_DST_LDS) != 0, ul = op.flags & MF_U_LDS;
    if (ctemp >= 64) {
        const int nwo = ctemp >> 3;  // multiple of 8
        if constexpr (NS >= 2) {
            // chunks of 4 words of both sets: the sets' loads are in flight together
            for (int w0 = 0; w0 < nwo; w0 += 4) {
                uint32_t A[NS][4], B[NS][4], ub[NS], ub2[NS];
#pragma unroll
                for (int s = 0; s < NS; ++s) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        A[s][k] = fg_word<RAW, SL>(P, M[s], op, y[s], src[s], w0 + k);
                        B[s][k] = fg_word<RAW, SL>(P, M[s], op, y[s], src[s], nwo + w0 + k);
                    }
                    ub[s] = ub2[s] = 0u;
                    if constexpr (ISG && LO) {  // 16 bits each, at bit 0 or 16 of their words (nwo a multiple of 8)
                        ub[s] = M[s].ld(ul, op.u_row + (w0 >> 3), usrc[s]) >> ((w0 & 4) << 2);
                        ub2[s] = M[s].ld(ul, op.u_row + ((nwo + w0) >> 3), usrc[s]) >> ((w0 & 4) << 2);
                    } else if constexpr (ISG) {
                        ub[s] = M[s].ld(ul, op.u_row + (w0 >> 2), usrc[s]);
                    }
                }
#pragma unroll
                for (int s = 0; s < NS; ++s)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if constexpr (LO) {
                            M[s].st(dl, op.dst_row + w0 + k, lane,
                                    LT ? lut_lds<8, ISG, 0, true, true>(A[s][k], B[s][k], ub[s] >> (k << 2), ub2[s] >> (k << 2))
                                       : lut_vec<8, true, true>(T, A[s][k], B[s][k], ub[s] >> (k << 2), ub2[s] >> (k << 2)));
                            continue;
                        }
                        M[s].st(dl, op.dst_row + w0 + k, lane,
                                LT ? lut_lds<8, ISG>(A[s][k], B[s][k], ub[s] >> (k << 3))
                                   : lut_vec<8>(T, A[s][k], B[s][k], ub[s] >> (k << 3)));
                    }
            }
        } else {
            for (int w0 = 0; w0 < nwo; w0 += 8) {
                uint32_t A[8], B[8], ub[2] = {0u, 0u};
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    A[k] = fg_word<RAW, SL>(P, M[0], op, y[0], src[0], w0 + k);
                    B[k] = fg_word<RAW, SL>(P, M[0], op, y[0], src[0], nwo + w0 + k);
                }
                if (ISG && LO) {  // u bits 4 w0 .. and 4 (nwo + w0) ..: one word each
                    ub[0] = M[0].ld(ul, op.u_row + (w0 >> 3), usrc[0]);
                    ub[1] = M[0].ld(ul, op.u_row + ((nwo + w0) >> 3), usrc[0]);
                } else if (ISG) {
                    ub[0] = M[0].ld(ul, op.u_row + (w0 >> 2), usrc[0]);
                    ub[1] = M[0].ld(ul, op.u_row + (w0 >> 2) + 1, usrc[0]);
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if constexpr (LO) {
                        M[0].st(dl, op.dst_row + w0 + k, lane, lut_vec<8, true, true>(T, A[k], B[k], ub[0] >> (k << 2), ub[1] >> (k << 2)));
                        continue;
                    }
                    M[0].st(dl, op.dst_row + w0 + k, lane, lut_vec<8>(T, A[k], B[k], ub[k >> 2] >> ((k & 3) << 3)));
                }
            }
        }
    } else if (ctemp >= 8) {
        const int nwo = ctemp >> 3;  // 1, 2 or 4
        uint32_t A[NS][4], B[NS][4], ub[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                A[s][k] = B[s][k] = 0u;
                if (k < nwo) {
                    A[s][k] = fg_word<RAW, SL>(P, M[s], op, y[s], src[s], k);
                    B[s][k] = fg_word<RAW, SL>(P, M[s], op, y[s], src[s], nwo + k);
                }
            }
            ub[s] = ISG ? M[s].ld(ul, op.u_row, usrc[s]) : 0u;
        }
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < nwo) {
                    if constexpr (LO) {  // U[d+1] is one word: bits 4k .. and 4 (nwo + k) ..
                        const uint32_t h2 = ub[s] >> (nwo << 2);
                        M[s].st(dl, op.dst_row + k, lane,
                                LT ? lut_lds<8, ISG, 0, true, true>(A[s][k], B[s][k], ub[s] >> (k << 2), h2 >> (k << 2))
                                   : lut_vec<8, true, true>(T, A[s][k], B[s][k], ub[s] >> (k << 2), h2 >> (k << 2)));
                        continue;
                    }
                    M[s].st(dl, op.dst_row + k, lane,
                            LT ? lut_lds<8, ISG>(A[s][k], B[s][k], ub[s] >> (k << 3))
                               : lut_vec<8>(T, A[s][k], B[s][k], ub[s] >> (k << 3)));
                }
    } else {  // ctemp in {2, 4}: the whole depth-d node (a then b) is one word
        uint32_t W[NS], ub[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            W[s] = fg_word<RAW, SL>(P, M[s], op, y[s], src[s], 0, 2 * ctemp);
            ub[s] = ISG ? M[s].ld(ul, op.u_row, usrc[s]) : 0u;
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const uint32_t out = ctemp == 4 ? lut_vec<4>(T, W[s], W[s] >> 16, ub[s]) : lut_vec<2>(T, W[s], W[s] >> 8, ub[s]);
            M[s].st(dl, op.dst_row, lane, out);
        }
    }
}

// f / g op with its left child's f folded in (MF_FF, fuse_descent in
// qpd_capi.hip): SCLLUTDecoder.cpp:83-89 / :157-164 at depth d, then :83-89
// at depth d+1.  Word u of S[d+2] is f(word u, word u + nwc) of S[d+1], both
// produced by this lane, so the child's inputs come from registers instead of
// a re-read of the row just stored (S[d+1] is still stored: the child's g
// reads it later).  Chunks of two S[d+2] words per set; S[d] in the slab.
// The op's table is staged at tb, the child's f table at tb + 512 (lut_lds).
// LO (rows in lookup order): the same words are read and written; S[d+1]'s words u and
// u + nwc, in lookup order, are the index words of S[d+2]'s word u as they lie.
template <bool ISG, int DL, int CDL, int NS, bool LO = false>
__device__ __forceinline__ void ff_op(const Mem (&M)[NS], const MOp &op, const int (&src)[NS], const int (&usrc)[NS],
                                      const uint8_t *tb, int lane) {
    const int nwo = op.cnt >> 3, nwc = nwo >> 1;  // nwc even (op.cnt >= 32)
    const bool ul = op.flags & MF_U_LDS;
    if constexpr (LO) {
        for (int u0 = 0; u0 < nwc; u0 += 2) {
            // u bits of word w: 4w .. 4w+3 and 4 (nwo + w) ..; the chunk's words u0, u0 + 1 (u0
            // even: one u word and shift) and nwc + u0, nwc + u0 + 1
            uint32_t A[NS][4], B[NS][4], ua[NS][2], ub[NS][2], X[NS][4];
#pragma unroll
            for (int s = 0; s < NS; ++s) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int w = (k < 2 ? 0 : nwc) + u0 + (k & 1);
                    A[s][k] = M[s].ld(false, op.src_row + w, src[s]);
                    B[s][k] = M[s].ld(false, op.src_row + nwo + w, src[s]);
                }
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    ua[s][h] = ub[s][h] = 0u;
                    if (ISG) {
                        const int w = (h ? nwc : 0) + u0;
                        ua[s][h] = M[s].ld(ul, op.u_row + (w >> 3), usrc[s]) >> ((w & 7) << 2);
                        ub[s][h] = M[s].ld(ul, op.u_row + ((nwo + w) >> 3), usrc[s]) >> (((nwo + w) & 7) << 2);
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < NS; ++s)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int w = (k < 2 ? 0 : nwc) + u0 + (k & 1);
                    X[s][k] = lut_lds<8, ISG, 0, true, true>(A[s][k], B[s][k], ua[s][k >> 1] >> ((k & 1) << 2),
                                                             ub[s][k >> 1] >> ((k & 1) << 2));
                    M[s].st(DL != 0, op.dst_row + w, lane, X[s][k]);
                }
#pragma unroll
            for (int s = 0; s < NS; ++s)
#pragma unroll
                for (int k = 0; k < 2; ++k)
                    M[s].st(CDL != 0, op.r_row + u0 + k, lane, lut_lds<8, false, 512, true, true>(X[s][k], X[s][k + 2], 0u));
        }
        return;
    }
    for (int u0 = 0; u0 < nwc; u0 += 2) {
        uint32_t A[NS][4], B[NS][4], ub[NS][2], X[NS][4];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int w = (k < 2 ? 0 : nwc) + u0 + (k & 1);
                A[s][k] = M[s].ld(false, op.src_row + w, src[s]);
                B[s][k] = M[s].ld(false, op.src_row + nwo + w, src[s]);
            }
            ub[s][0] = ub[s][1] = 0u;
            if (ISG) {
                ub[s][0] = M[s].ld(ul, op.u_row + (u0 >> 2), usrc[s]);
                ub[s][1] = M[s].ld(ul, op.u_row + ((nwc + u0) >> 2), usrc[s]);
            }
        }
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int w = (k < 2 ? 0 : nwc) + u0 + (k & 1);
                X[s][k] = lut_lds<8, ISG>(A[s][k], B[s][k], ub[s][k >> 1] >> ((w & 3) << 3));
                M[s].st(DL != 0, op.dst_row + w, lane, X[s][k]);
            }
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int k = 0; k < 2; ++k)
                M[s].st(CDL != 0, op.r_row + u0 + k, lane, lut_lds<8, false, 512>(X[s][k], X[s][k + 2], 0u));
    }
}

// Bit i of b (i < 8) -> nibble i all ones.
__device__ __forceinline__ uint32_t nib_mask(uint32_t b) {
    b &= 0xFFu;
    b = (b | (b << 12)) & 0x000F000Fu;
    b = (b | (b << 6)) & 0x03030303u;
    b = (b | (b << 3)) & 0x11111111u;
    return b * 15u;
}

// Root g in pre-mode (MF_GSEL; SCLLUTDecoder.cpp:157-164 at depth 0): the
// pre-pass row holds g(y, 0) and g(y, 1) of every root position, so the
// path's symbols are a nibble select by its left-half partial sums u.
// LO (rows in lookup order): the pre-pass rows and S[1] are in that order, so word w's
// high nibbles select by u bits 4w .. 4w+3 and its low ones by bits 4 (nwo + w) ..
template <int NS, bool LO = false>
__device__ __forceinline__ void gsel_op(const Mem (&M)[NS], const MOp &op, const int32_t *const (&y)[NS],
                                        const int (&usrc)[NS], int lane) {
    const int nwo = op.cnt >> 3;  // 1, 2, 4 or a multiple of 8
    const bool dl = op.flags & MF_DST_LDS, ul = op.flags & MF_U_LDS;
    if constexpr (LO) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const uint32_t *g = (const uint32_t *)y[s] + op.src_row;
            for (int w0 = 0; w0 < nwo; w0 += 8) {
                uint32_t g0[8], g1[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    g0[k] = g1[k] = 0u;
                    if (k == 0 || w0 + k < nwo) {
                        g0[k] = g[w0 + k];
                        g1[k] = g[nwo + w0 + k];
                    }
                }
                // nwo < 8: U[1] is one word (w0 = 0), the low nibbles' bits from 4 nwo on
                const uint32_t ua = M[s].ld(ul, op.u_row + (w0 >> 3), usrc[s]);
                const uint32_t ub = M[s].ld(ul, op.u_row + ((nwo + w0) >> 3), usrc[s]) >> ((nwo << 2) & 31);
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (k == 0 || w0 + k < nwo) {
                        const uint32_t m = ((byte_bits4((ua >> (k << 2)) & 15u) << 4) | byte_bits4((ub >> (k << 2)) & 15u)) * 15u;
                        M[s].st(dl, op.dst_row + w0 + k, lane, g0[k] ^ ((g0[k] ^ g1[k]) & m));
                    }
            }
        }
        return;
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const uint32_t *g = (const uint32_t *)y[s] + op.src_row;  // g(y, 0) words; g(y, 1) at + nwo
        for (int w0 = 0; w0 < nwo; w0 += 8) {
            uint32_t g0[8], g1[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                g0[k] = g1[k] = 0u;
                if (k == 0 || w0 + k < nwo) {
                    g0[k] = g[w0 + k];
                    g1[k] = g[nwo + w0 + k];
                }
            }
            const uint32_t u0 = M[s].ld(ul, op.u_row + (w0 >> 2), usrc[s]);
            const uint32_t u1 = nwo - w0 > 4 ? M[s].ld(ul, op.u_row + (w0 >> 2) + 1, usrc[s]) : 0u;
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (k == 0 || w0 + k < nwo) {
                    const uint32_t m = nib_mask((k < 4 ? u0 : u1) >> ((k & 3) << 3));
                    M[s].st(dl, op.dst_row + w0 + k, lane, g0[k] ^ ((g0[k] ^ g1[k]) & m));
                }
        }
    }
}

// Prefetch of the per-op operands held in registers.
struct Pre {
    uint32_t T;   // f or g table dword of this lane
    uint32_t T2;  // MF_BFG: the folded parent op's table dword
    double V;     // leaf: vcl row entry of this lane (lanes < v)
};

__device__ __forceinline__ Pre fetch_pre(const FastPlan &P, const MOp &op, int lane, int vlane) {
    Pre p;
    p.T = p.T2 = 0;
    p.V = 0;
    if (op.type == OP_F || op.type == OP_LEAF_L) p.T = tab_ld(P.f_tab, op.tab * QPD_EXP_TABMUL, lane & 31);
    if ((op.type == OP_G && !(op.flags & MF_GSEL)) || op.type == OP_LEAF_R) p.T = tab_ld(P.g_tab, op.tab * QPD_EXP_TABMUL, lane);
    if ((op.type == OP_F || op.type == OP_G) && (op.flags & MF_FF)) p.T2 = tab_ld(P.f_tab, op.tab2 * QPD_EXP_TABMUL, lane & 31);
    if (op.type == OP_BOT3) {
        p.T = tab_ld(P.f_tab, op.tab * QPD_EXP_TABMUL * 32, lane & 31);
        if (op.flags & MF_BFG)
            p.T2 = (op.flags & MF_BG) ? tab_ld(P.g_tab, op.tab2 * QPD_EXP_TABMUL, lane)
                                      : tab_ld(P.f_tab, op.tab2 * QPD_EXP_TABMUL, lane & 31);
    }
    if (op.type == OP_LEAF_L || op.type == OP_LEAF_R) p.V = P.vcl[op.vrow + vlane];
    if (op.type >= OP_R0 && op.type <= OP_SPC && (op.flags & MF_SFG))  // the folded parent's table (tab)
        p.T2 = (op.flags & MF_SGG) ? tab_ld(P.g_tab, op.tab, lane) : tab_ld(P.f_tab, op.tab, lane & 31);
    return p;
}

}  // namespace qpd
