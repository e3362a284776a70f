// Device harness of the fast engine's table lookups and the f / g ops made of them: small
// kernels that call the real device functions of qpd_fast_lookup.hpp -- lut4, lut_vec,
// lut_byte, stage_tab + lut_lds, the SWAR helpers, the channel readers, fg_op, fg_chan_op,
// ff_op, gsel_op -- and qpd_fast_pre.hpp's root_pre_kernel, on operands, tables and rows the
// caller chooses.  One wave per block, as the decode kernel.  Tables arrive raw
// (tf[a * v + b], tg[u * v * v + a * v + b]) and are packed by the product's own
// qpd_plan::pack_tables; the harness restates no lookup and no layout.
//
// lut_lds addresses LDS through a constant (TOFF), so every kernel here uses dynamic LDS
// only, the staged tables first: [tables 768 B] [canary 64 words] [rows] [canary 64 words].
// Every entry point checks hipFuncGetAttributes(...).sharedSizeBytes == 0 before it
// launches (error -2 otherwise), as check_no_static_lds does for the product.
//
// The op kernels run one op record per launch on a Mem whose LDS rows lie between the two
// canary rows and whose slab rows sit behind a buffer descriptor of exactly the block's slab
// bytes: a wrong slab row reads zeros or drops the store.  The caller hands in the whole LDS
// and slab images and gets both back after the op, so it can check every row: the
// destination in full, all others unchanged.  Every run reports per block that the canaries
// (bit 0) and the rows the op reads (bit 1) are intact.
//
// A checker, not a stress tool: every entry point validates its arguments before any launch
// and returns -1 for what the decode kernels could not run.
#include "qpd_fast_pre.hpp"
#include "qpd_plan.hpp"

#include <cstring>
#include <vector>

#ifndef QPD_LK_BUILD_ID
#define QPD_LK_BUILD_ID "unstamped"
#endif

namespace {

using qpd::FastPlan;
using qpd::Mem;
using qpd::MOp;

enum Fn {
    F_LUT4 = 0,      // lut4(T, b)
    F_VEC2 = 1,      // lut_vec<2>(T, a, b, h)
    F_VEC4 = 2,
    F_VEC8 = 3,
    F_VEC8IL = 4,    // lut_vec<8, true>
    F_BYTE2 = 5,     // lut_byte<2, false, false>(T, a)
    F_BYTE2H = 6,    // lut_byte<2, false, true>(T, a, h)
    F_BYTE4 = 7,     // lut_byte<4, true, false>(T, a)
    F_BYTE4H = 8,    // lut_byte<4, true, true>(T, a, h)
    F_LDS8F = 9,     // stage_tab, lut_lds<8, false>(a, b, h)
    F_LDS8G = 10,    // stage_tab(gtab_dw), lut_lds<8, true>
    F_LDS8GIL = 11,  // ... lut_lds<8, true, 0, true>
    F_LDS8F512 = 12, // stage_tab at tb + 512, lut_lds<8, false, 512>
    F_INTERLEAVE = 13,
    F_ILNIB = 14,    // il_nib<8>(a & 7) | il_nib<4>(a & 3) << 8 | il_nib<2>(a & 1) << 16
    F_HALF2 = 15,
    F_HALF4 = 16,
    F_PACK4 = 17,
    F_N2B4 = 18,
    F_NIBMASK = 19,
    F_POLAR = 20,
    F_COUNT
};
enum Chan { C_W8_I32_VEC = 0, C_W8_I32 = 1, C_W8_U8_VEC = 2, C_W8_U8 = 3, C_WORD_I32 = 4, C_WORD_U8 = 5, C_SMALL = 6, C_COUNT };
enum Kind { K_FG = 0, K_FGP = 1, K_CHAN = 2, K_FF = 3, K_GSEL = 4, K_COUNT };

constexpr int kTabWords = 192;  // the staged tables: the op's (512 B) and the folded child's f (256 B)
constexpr int kCanary = 64;
constexpr uint32_t kCanaryWord = 0xC0DE5E1Fu;
constexpr int kRowsAt = kTabWords + kCanary;  // word offset of the wave's LDS row 0
constexpr int kMaxLdsBytes = 64 * 1024;

__device__ __forceinline__ void lds_head(uint32_t *lds, int back, int lane) {
    for (int i = lane; i < kTabWords; i += 64) lds[i] = 0u;
    lds[kTabWords + lane] = kCanaryWord ^ (uint32_t)lane;
    lds[back + lane] = ~kCanaryWord ^ (uint32_t)lane;
}

__device__ __forceinline__ bool lds_canaries(const uint32_t *lds, int back, int lane) {
    const bool can = lds[kTabWords + lane] == (kCanaryWord ^ (uint32_t)lane) && lds[back + lane] == (~kCanaryWord ^ (uint32_t)lane);
    return __builtin_amdgcn_ballot_w64(!can) == 0;
}

// tsel: 0 the f table of node 0 (lanes & 31), 1 the g table of node 0, 2 the f tables of nodes 0 and 1
// as one register row (BOT3's Tf12: the second table is the upper half)
__device__ __forceinline__ uint32_t table_reg(const uint32_t *ft, const uint32_t *gt, int tsel, int lane) {
    return tsel == 0 ? ft[lane & 31] : tsel == 1 ? gt[lane] : ft[lane];
}

template <int FN>
__global__ __launch_bounds__(64) void prim_kernel(const uint32_t *__restrict__ ft, const uint32_t *__restrict__ gt, int tsel,
                                                  const uint32_t *__restrict__ a, const uint32_t *__restrict__ b,
                                                  const uint32_t *__restrict__ h, uint32_t *__restrict__ out,
                                                  int32_t *__restrict__ ok) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_dyn[];
    const int lane = threadIdx.x;
    const size_t at = (size_t)blockIdx.x * 64 + lane;
    uint8_t *const tb = (uint8_t *)lds_dyn;
    lds_head(lds_dyn, kRowsAt, lane);
    __syncthreads();
    const uint32_t T = table_reg(ft, gt, tsel, lane);
    if constexpr (FN == F_LDS8F) qpd::stage_tab(tb, T, lane & 31);
    if constexpr (FN == F_LDS8G || FN == F_LDS8GIL) qpd::stage_tab(tb, T, qpd::gtab_dw(lane));
    if constexpr (FN == F_LDS8F512) qpd::stage_tab(tb + 512, T, lane & 31);
    __syncthreads();
    const uint32_t A = a[at], B = b[at], H = h[at];
    uint32_t r = 0;
    if constexpr (FN == F_LUT4) r = qpd::lut4(T, B);
    if constexpr (FN == F_VEC2) r = qpd::lut_vec<2>(T, A, B, H);
    if constexpr (FN == F_VEC4) r = qpd::lut_vec<4>(T, A, B, H);
    if constexpr (FN == F_VEC8) r = qpd::lut_vec<8>(T, A, B, H);
    if constexpr (FN == F_VEC8IL) r = qpd::lut_vec<8, true>(T, A, B, H);
    if constexpr (FN == F_BYTE2) r = qpd::lut_byte<2, false, false>(T, A);
    if constexpr (FN == F_BYTE2H) r = qpd::lut_byte<2, false, true>(T, A, H);
    if constexpr (FN == F_BYTE4) r = qpd::lut_byte<4, true, false>(T, A);
    if constexpr (FN == F_BYTE4H) r = qpd::lut_byte<4, true, true>(T, A, H);
    if constexpr (FN == F_LDS8F) r = qpd::lut_lds<8, false>(A, B, H);
    if constexpr (FN == F_LDS8G) r = qpd::lut_lds<8, true>(A, B, H);
    if constexpr (FN == F_LDS8GIL) r = qpd::lut_lds<8, true, 0, true>(A, B, H);
    if constexpr (FN == F_LDS8F512) r = qpd::lut_lds<8, false, 512>(A, B, H);
    if constexpr (FN == F_INTERLEAVE) r = qpd::nib_interleave8(A);
    if constexpr (FN == F_ILNIB)
        r = (uint32_t)qpd::il_nib<8>((int)(A & 7u)) | ((uint32_t)qpd::il_nib<4>((int)(A & 3u)) << 8) |
            ((uint32_t)qpd::il_nib<2>((int)(A & 1u)) << 16);
    if constexpr (FN == F_HALF2) r = qpd::half_bits2(A);
    if constexpr (FN == F_HALF4) r = qpd::half_bits4(A);
    if constexpr (FN == F_PACK4) r = qpd::nib_pack4(A);
    if constexpr (FN == F_N2B4) r = qpd::nib2byte4(A);
    if constexpr (FN == F_NIBMASK) r = qpd::nib_mask(A);
    if constexpr (FN == F_POLAR) r = qpd::polar_word(A);
    out[at] = r;
    __syncthreads();
    const bool can = lds_canaries(lds_dyn, kRowsAt, lane);
    if (lane == 0) ok[blockIdx.x] = can ? 3 : 2;
}

// One reader call per lane: symbols e0 .. e0 + cnt - 1 of buf, the lane's own error word.
template <int MODE>
__global__ __launch_bounds__(64) void chan_kernel(const void *__restrict__ buf, const int32_t *__restrict__ e0,
                                                  const int32_t *__restrict__ cnt, int v, uint32_t *__restrict__ out,
                                                  int32_t *__restrict__ err) {
    const size_t at = (size_t)blockIdx.x * 64 + threadIdx.x;
    const int e = e0[at], c = cnt[at];
    const int32_t *yi = (const int32_t *)buf;
    const uint8_t *yb = (const uint8_t *)buf;
    uint32_t r = 0;
    if constexpr (MODE == C_W8_I32_VEC) r = qpd::chan_word8(yi, e, true, v, err + at);
    if constexpr (MODE == C_W8_I32) r = qpd::chan_word8(yi, e, false, v, err + at);
    if constexpr (MODE == C_W8_U8_VEC) r = qpd::chan_word8(yb, e, true, v, err + at);
    if constexpr (MODE == C_W8_U8) r = qpd::chan_word8(yb, e, false, v, err + at);
    if constexpr (MODE == C_WORD_I32) r = qpd::chan_word(yi, e, c, v, err + at);
    if constexpr (MODE == C_WORD_U8) r = qpd::chan_word(yb, e, c, v, err + at);
    if constexpr (MODE == C_SMALL) r = qpd::chan_small(yi + e, c, v, err + at);
    out[at] = r;
}

struct OpArgs {
    MOp op;
    int32_t v, in_vec, gs, lds_rows, glb_rows, ystride;
    const uint32_t *ft, *gt;  // packed tables: f of nodes 0 (the op's) and 1 (the folded child's), g of node 0
    const int32_t *y;         // [blocks][NS][64 / gs][ystride] channel symbols or pre-pass rows
    const uint32_t *lds_in;   // [blocks][lds_rows][NS][64]
    uint32_t *lds_out;
    uint32_t *slab;           // [blocks][glb_rows][NS][64], in and out
    const uint8_t *srcf, *usrcf;  // [blocks][NS][64] pointer fields (slots inside the lane's group)
    int32_t *err;             // [blocks]
    int32_t *ok;              // [blocks]
};

// KIND K_FG: fg_op<ISG, true, NS, SL = X, DL = Y, LT>; K_FGP: fg_op<ISG, false, NS>; K_CHAN: fg_chan_op<ISG, NS>;
// K_FF: ff_op<ISG, DL = X, CDL = Y, NS>; K_GSEL: gsel_op<NS>.
template <int KIND, bool ISG, int NS, int X, int Y, bool LT>
__global__ __launch_bounds__(64) void op_kernel(OpArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_dyn[];
    const int lane = threadIdx.x, gl = lane & (a.gs - 1), gbase = lane - gl;
    const int nrow = NS * a.lds_rows * 64, back = kRowsAt + nrow;
    uint8_t *const tb = (uint8_t *)lds_dyn;
    uint32_t *const lds_rows = lds_dyn + kRowsAt;
    lds_head(lds_dyn, back, lane);
    const uint32_t *lin = a.lds_in + (size_t)blockIdx.x * nrow;
    for (int i = lane; i < nrow; i += 64) lds_rows[i] = lin[i];
    __syncthreads();
    FastPlan P{};
    P.v = a.v;
    P.in_vec = a.in_vec;
    P.err = a.err + blockIdx.x;
    Mem Mv[NS];
    uint32_t *const slab = a.slab + (size_t)blockIdx.x * NS * a.glb_rows * 64;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(slab, 0, NS * a.glb_rows * 256, 0x00020000);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        Mv[s].lds = lds_rows + s * 64;
        Mv[s].gp = slab + s * 64;
        Mv[s].rs = rs;
        Mv[s].so = s * 256;
        Mv[s].ns = NS;
    }
    const MOp op = a.op;
    const int gsh = __builtin_ctz(a.gs);
    const int32_t *yv[NS];
    int src[NS], usrc[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const size_t bs = (size_t)blockIdx.x * NS + s;
        yv[s] = a.y + (bs * (64 >> gsh) + (lane >> gsh)) * a.ystride;
        uint64_t ps = 0;  // every field the lane's own slot, then the two the op reads
        for (int d = 0; d < 16; ++d) ps |= (uint64_t)gl << (4 * d);
        ps = qpd::pset(ps, op.sh_src, a.srcf[bs * 64 + lane]);
        ps = qpd::pset(ps, op.sh_u, a.usrcf[bs * 64 + lane]);
        src[s] = gbase + qpd::pfield(ps, op.sh_src);
        usrc[s] = gbase + qpd::pfield(ps, op.sh_u);
    }
    const uint32_t T = ISG ? a.gt[lane] : a.ft[lane & 31];
    if constexpr (KIND == K_FF) {
        qpd::stage_tab(tb, T, ISG ? qpd::gtab_dw(lane) : (lane & 31));
        qpd::stage_tab(tb + 512, a.ft[32 + (lane & 31)], lane & 31);
        __syncthreads();
        qpd::ff_op<ISG, X, Y, NS>(Mv, op, src, usrc, tb, lane);
    } else if constexpr (KIND == K_FG) {
        if constexpr (LT) {
            qpd::stage_tab(tb, T, ISG ? qpd::gtab_dw(lane) : (lane & 31));
            __syncthreads();
        }
        qpd::fg_op<ISG, true, NS, X, Y, LT>(P, Mv, op, yv, src, usrc, T, lane, tb);
    } else if constexpr (KIND == K_FGP) {
        qpd::fg_op<ISG, false, NS>(P, Mv, op, yv, src, usrc, T, lane);
    } else if constexpr (KIND == K_CHAN) {
        qpd::fg_chan_op<ISG, NS>(P, Mv, op, yv, usrc, T, lane);
    } else {
        qpd::gsel_op<NS>(Mv, op, yv, usrc, lane);
    }
    __syncthreads();
    uint32_t *lout = a.lds_out + (size_t)blockIdx.x * nrow;
    for (int i = lane; i < nrow; i += 64) lout[i] = lds_rows[i];
    const bool can = lds_canaries(lds_dyn, back, lane);
    if (lane == 0) a.ok[blockIdx.x] = can ? 1 : 0;
}

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

#define LK_TRY(x) \
    if ((e = (x)) != hipSuccess) return (int)e

int upload(DevBuf &d, const void *h, size_t bytes) {
    hipError_t e;
    LK_TRY(hipMalloc(&d.p, bytes ? bytes : 1));
    if (bytes) LK_TRY(hipMemcpy(d.p, h, bytes, hipMemcpyHostToDevice));
    return 0;
}

int alloc_fill(DevBuf &d, size_t bytes, int fill) {
    hipError_t e;
    LK_TRY(hipMalloc(&d.p, bytes ? bytes : 1));
    LK_TRY(hipMemset(d.p, fill, bytes ? bytes : 1));
    return 0;
}

// lut_lds reaches the tables through a constant LDS offset: nothing static may lie before them
int no_static_lds(const void *fn) {
    hipFuncAttributes at;
    hipError_t e;
    LK_TRY(hipFuncGetAttributes(&at, fn));
    return at.sharedSizeBytes == 0 ? 0 : -2;
}

bool raw_ok(const uint8_t *t, size_t n) {  // a table entry is a nibble
    for (size_t i = 0; i < n; ++i)
        if (t[i] >= 16) return false;
    return true;
}

// tf: [2][v][v] (nodes 0 and 1), tg: [2][v][v] (node 0: u = 0, u = 1) -> the product's packed tables of a
// code of N = 8 whose nodes 0 and 1 are plain (not leaf pairs): ft[0..31], ft[32..63], gt[0..63]
int pack(int v, const uint8_t *tf, const uint8_t *tg, std::vector<uint32_t> &ft, std::vector<uint32_t> &gt) {
    if (v < 2 || v > 16 || !tf || !tg) return -1;
    if (!raw_ok(tf, (size_t)2 * v * v) || !raw_ok(tg, (size_t)2 * v * v)) return -1;
    static const int32_t f_base[7] = {0, 1, 1, 1, 1, 1, 1}, g_base[7] = {0, 0, 0, 0, 0, 0, 0};
    qpd_config c;
    std::memset(&c, 0, sizeof c);
    c.N = 8;
    c.v = v;
    c.lut_f = tf;
    c.lut_f_count = 2;
    c.f_base = f_base;
    c.lut_g = tg;
    c.lut_g_count = 1;
    c.g_base = g_base;
    qpd_plan::pack_tables(c, ft, gt);
    return 0;
}

template <int FN>
const void *prim_fn() {
    return reinterpret_cast<const void *>(&prim_kernel<FN>);
}

const void *prim_pick(int fn) {
    switch (fn) {
#define LK_P(F) \
    case F:     \
        return prim_fn<F>();
        LK_P(F_LUT4) LK_P(F_VEC2) LK_P(F_VEC4) LK_P(F_VEC8) LK_P(F_VEC8IL) LK_P(F_BYTE2) LK_P(F_BYTE2H) LK_P(F_BYTE4)
        LK_P(F_BYTE4H) LK_P(F_LDS8F) LK_P(F_LDS8G) LK_P(F_LDS8GIL) LK_P(F_LDS8F512) LK_P(F_INTERLEAVE) LK_P(F_ILNIB)
        LK_P(F_HALF2) LK_P(F_HALF4) LK_P(F_PACK4) LK_P(F_N2B4) LK_P(F_NIBMASK) LK_P(F_POLAR)
#undef LK_P
    }
    return nullptr;
}

const void *chan_pick(int mode) {
    switch (mode) {
#define LK_C(M) \
    case M:     \
        return reinterpret_cast<const void *>(&chan_kernel<M>);
        LK_C(C_W8_I32_VEC) LK_C(C_W8_I32) LK_C(C_W8_U8_VEC) LK_C(C_W8_U8) LK_C(C_WORD_I32) LK_C(C_WORD_U8) LK_C(C_SMALL)
#undef LK_C
    }
    return nullptr;
}

template <int KIND, bool ISG, int NS>
const void *op_pick_xy(int x, int y, bool lt) {
    if constexpr (KIND == K_FG) {
#define LK_O(X_, Y_) \
    if (x == X_ && y == Y_) \
        return lt ? reinterpret_cast<const void *>(&op_kernel<KIND, ISG, NS, X_, Y_, true>) \
                  : reinterpret_cast<const void *>(&op_kernel<KIND, ISG, NS, X_, Y_, false>);
        LK_O(0, 0) LK_O(0, 1) LK_O(1, 1)
#undef LK_O
        return nullptr;
    } else if constexpr (KIND == K_FF) {
#define LK_O(X_, Y_) \
    if (x == X_ && y == Y_) return reinterpret_cast<const void *>(&op_kernel<KIND, ISG, NS, X_, Y_, false>);
        LK_O(0, 0) LK_O(0, 1) LK_O(1, 1)
#undef LK_O
        return nullptr;
    } else {
        return reinterpret_cast<const void *>(&op_kernel<KIND, ISG, NS, 0, 0, false>);
    }
}

template <int KIND>
const void *op_pick_kind(bool isg, int ns, int x, int y, bool lt) {
    if (isg) return ns == 2 ? op_pick_xy<KIND, true, 2>(x, y, lt) : op_pick_xy<KIND, true, 1>(x, y, lt);
    return ns == 2 ? op_pick_xy<KIND, false, 2>(x, y, lt) : op_pick_xy<KIND, false, 1>(x, y, lt);
}

const void *op_pick(int kind, bool isg, int ns, int x, int y, bool lt) {
    switch (kind) {
        case K_FG: return op_pick_kind<K_FG>(isg, ns, x, y, lt);
        case K_FGP: return op_pick_kind<K_FGP>(isg, ns, x, y, lt);
        case K_CHAN: return op_pick_kind<K_CHAN>(isg, ns, x, y, lt);
        case K_FF: return op_pick_kind<K_FF>(isg, ns, x, y, lt);
        case K_GSEL: return ns == 2 ? op_pick_xy<K_GSEL, true, 2>(0, 0, false) : op_pick_xy<K_GSEL, true, 1>(0, 0, false);
    }
    return nullptr;
}

bool pow2(int x) { return x > 0 && (x & (x - 1)) == 0; }

struct Span {
    bool lds;
    int row, rows;
};

bool disjoint(const Span &a, const Span &b) { return a.lds != b.lds || a.row + a.rows <= b.row || b.row + b.rows <= a.row; }

}  // namespace

extern "C" {

const char *qpd_lk_build_id() {
    static const char tag[] = "qpd-lkh-build-id:" QPD_LK_BUILD_ID;
    return tag + 17;
}

// The compile switches this library was built with.
void qpd_lk_variant(int32_t *vec_chain, int32_t *gswz, int32_t *lutmask) {
    *vec_chain = QPD_VEC_CHAIN;
    *gswz = QPD_GSWZ;
    *lutmask = QPD_EXP_LUTMASK;
}

// Function `fn` on n lanes (a multiple of 64), one result word per lane.  tsel: the table register row
// (0 f of node 0, 1 g, 2 both f tables).  ok: [n / 64], bit 0 = the block's canaries are intact.
int qpd_lk_prim(int fn, int tsel, int v, const uint8_t *tf, const uint8_t *tg, int n, const uint32_t *a, const uint32_t *b,
                const uint32_t *h, uint32_t *out, int32_t *ok) {
    if (fn < 0 || fn >= F_COUNT || tsel < 0 || tsel > 2 || n < 64 || (n & 63) || n > (1 << 22)) return -1;
    if (!a || !b || !h || !out || !ok) return -1;
    if ((fn == F_LDS8F || fn == F_LDS8F512) && tsel != 0) return -1;
    if ((fn == F_LDS8G || fn == F_LDS8GIL) && tsel != 1) return -1;
    std::vector<uint32_t> ft, gt;
    if (pack(v, tf, tg, ft, gt)) return -1;
    for (int i = 0; i < n; ++i) {  // the functions' domains
        if (fn == F_LUT4 && b[i] >= 512u) return -1;
        if (fn == F_HALF2 && a[i] >= 4u) return -1;
        if (fn == F_HALF4 && a[i] >= 16u) return -1;
        if (fn == F_PACK4 && (a[i] & 0xF0F0F0F0u)) return -1;
        if (fn == F_N2B4 && a[i] >= 65536u) return -1;
    }
    const void *k = prim_pick(fn);
    if (!k) return -1;
    int rc;
    if ((rc = no_static_lds(k))) return rc;
    const size_t bytes = (size_t)n * 4;
    DevBuf dft, dgt, da, db, dh, dout, dok;
    hipError_t e;
    if ((rc = upload(dft, ft.data(), 64 * 4))) return rc;
    if ((rc = upload(dgt, gt.data(), 64 * 4))) return rc;
    if ((rc = upload(da, a, bytes))) return rc;
    if ((rc = upload(db, b, bytes))) return rc;
    if ((rc = upload(dh, h, bytes))) return rc;
    if ((rc = alloc_fill(dout, bytes, 0xEE))) return rc;
    if ((rc = alloc_fill(dok, (size_t)(n / 64) * 4, 0))) return rc;
    const uint32_t *aft = (const uint32_t *)dft.p, *agt = (const uint32_t *)dgt.p, *aa = (const uint32_t *)da.p,
                   *ab = (const uint32_t *)db.p, *ah = (const uint32_t *)dh.p;
    uint32_t *ao = (uint32_t *)dout.p;
    int32_t *ak = (int32_t *)dok.p;
    int ats = tsel;
    void *args[] = {&aft, &agt, &ats, &aa, &ab, &ah, &ao, &ak};
    LK_TRY(hipLaunchKernel(k, dim3(n / 64), dim3(64), args, (kRowsAt + kCanary) * 4, nullptr));
    LK_TRY(hipDeviceSynchronize());
    LK_TRY(hipMemcpy(out, dout.p, bytes, hipMemcpyDeviceToHost));
    LK_TRY(hipMemcpy(ok, dok.p, (size_t)(n / 64) * 4, hipMemcpyDeviceToHost));
    return 0;
}

// Channel reader `mode` on n lanes: lane i reads symbols e0[i] .. e0[i] + cnt[i] - 1 of buf (size elements
// of int32 or uint8) and has its own error word err[i].  The buffer's base is 256-byte aligned, so e0 decides
// the alignment: the vec readers take e0 a multiple of 4 (int32) or 8 (uint8) only.
int qpd_lk_chan(int mode, int v, int n, int64_t size, const void *buf, const int32_t *e0, const int32_t *cnt, uint32_t *out,
                int32_t *err) {
    if (mode < 0 || mode >= C_COUNT || v < 2 || v > 16 || n < 64 || (n & 63) || n > (1 << 22) || size < 1) return -1;
    if (!buf || !e0 || !cnt || !out || !err) return -1;
    const bool u8 = mode == C_W8_U8_VEC || mode == C_W8_U8 || mode == C_WORD_U8;
    for (int i = 0; i < n; ++i) {
        const bool w8 = mode <= C_W8_U8;
        if (w8 ? cnt[i] != 8 : (cnt[i] < 0 || cnt[i] > 8)) return -1;
        if (e0[i] < 0 || (int64_t)e0[i] + cnt[i] > size) return -1;
        if (mode == C_W8_I32_VEC && (e0[i] & 3)) return -1;
        if (mode == C_W8_U8_VEC && (e0[i] & 7)) return -1;
    }
    const void *k = chan_pick(mode);
    if (!k) return -1;
    DevBuf dbuf, de, dc, dout, derr;
    int rc;
    hipError_t e;
    if ((rc = upload(dbuf, buf, (size_t)size * (u8 ? 1 : 4)))) return rc;
    if ((rc = upload(de, e0, (size_t)n * 4))) return rc;
    if ((rc = upload(dc, cnt, (size_t)n * 4))) return rc;
    if ((rc = alloc_fill(dout, (size_t)n * 4, 0xEE))) return rc;
    if ((rc = alloc_fill(derr, (size_t)n * 4, 0))) return rc;
    const void *ab = dbuf.p;
    const int32_t *ae = (const int32_t *)de.p, *ac = (const int32_t *)dc.p;
    uint32_t *ao = (uint32_t *)dout.p;
    int32_t *ar = (int32_t *)derr.p;
    int av = v;
    void *args[] = {&ab, &ae, &ac, &av, &ao, &ar};
    LK_TRY(hipLaunchKernel(k, dim3(n / 64), dim3(64), args, 0, nullptr));
    LK_TRY(hipDeviceSynchronize());
    LK_TRY(hipMemcpy(out, dout.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    LK_TRY(hipMemcpy(err, derr.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
}

// One op on nblocks one-wave blocks of nsets frame sets.
//   kind, isg: the op (enum Kind); lt: K_FG's LT; pre: K_FGP reads MF_PRE words of y instead of a row
//   cnt: op.cnt; gs: lanes per frame (the pointer fields' group)
//   spaces: bit 0 S[d] in LDS, bit 1 the destination in LDS, bit 2 the U rows in LDS, bit 3 (K_FF) S[d+2] in LDS
//   rows: src_row, dst_row, u_row, r_row
//   y: [nblocks][nsets][64 / gs][ystride] int32 words; lds / slab: [nblocks][rows][nsets][64], in and out
//   srcf, usrcf: [nblocks][nsets][64] slots < gs; err, ok: [nblocks] (ok bit 0 canaries, bit 1 read rows intact)
int qpd_lk_op(int kind, int isg, int lt, int pre, int cnt, int v, int in_vec, int gs, int nsets, int nblocks, int spaces,
              const int32_t *rows, int lds_rows, int glb_rows, int ystride, const uint8_t *tf, const uint8_t *tg,
              const int32_t *y, uint32_t *lds, uint32_t *slab, const uint8_t *srcf, const uint8_t *usrcf, int32_t *err,
              int32_t *ok) {
    if (kind < 0 || kind >= K_COUNT || nsets < 1 || nsets > 2 || nblocks < 1 || nblocks > 4096) return -1;
    if (!pow2(gs) || gs > 16 || lds_rows < 1 || glb_rows < 1 || ystride < 1 || (spaces & ~15)) return -1;
    if (!rows || !y || !lds || !slab || !srcf || !usrcf || !err || !ok) return -1;
    if (!pow2(cnt) || cnt < 2 || cnt > 256) return -1;
    isg = isg ? 1 : 0;
    if (kind == K_GSEL) isg = 1;
    const bool sl = spaces & 1, dl = spaces & 2, ul = spaces & 4, cdl = spaces & 8;
    const int nwo = cnt >= 8 ? cnt >> 3 : 1, nwc = nwo >> 1;
    const bool rowsrc = kind == K_FG || kind == K_FF || (kind == K_FGP && !pre);
    if (kind == K_FG && cnt < 8) return -1;
    if (kind == K_FGP && (pre ? cnt < 8 : cnt > 4)) return -1;  // row words below 8 symbols; pre-pass rows from 8 on
    if (kind == K_FF && (cnt < 32 || sl || (dl && !cdl))) return -1;
    if (kind == K_GSEL && cnt < 8) return -1;
    if (kind != K_FF && cdl) return -1;
    if (kind != K_FG && lt) return -1;
    if (rowsrc && sl && !dl) return -1;  // the planner never puts S[d + 1] in the slab below an S[d] in LDS
    if (!rowsrc && sl) return -1;
    if (!isg && ul) return -1;
    if (in_vec && (kind != K_CHAN || (ystride & 3))) return -1;
    if (kind == K_CHAN && ystride < 2 * cnt) return -1;
    if ((kind == K_GSEL || (kind == K_FGP && pre)) && (rows[0] < 0 || ystride < rows[0] + 2 * nwo)) return -1;
    const size_t nrow = (size_t)nsets * lds_rows * 64;
    if ((kRowsAt + kCanary + nrow) * 4 > (size_t)kMaxLdsBytes) return -1;
    // every row the op touches lies inside its space, and nothing it writes overlaps what it reads
    std::vector<Span> reads, writes;
    if (rowsrc) reads.push_back({sl, rows[0], cnt >= 8 ? 2 * nwo : 1});
    if (isg) reads.push_back({ul, rows[2], (nwo + 3) / 4});
    writes.push_back({dl, rows[1], nwo});
    if (kind == K_FF) writes.push_back({cdl, rows[3], nwc});
    for (const std::vector<Span> *sv : {&reads, &writes})
        for (const Span &s : *sv)
            if (s.row < 0 || s.rows < 1 || s.row + s.rows > (s.lds ? lds_rows : glb_rows)) return -1;
    for (const Span &w : writes)
        for (const Span &r : reads)
            if (!disjoint(w, r)) return -1;
    if (writes.size() == 2 && !disjoint(writes[0], writes[1])) return -1;
    const size_t nbs = (size_t)nblocks * nsets;
    for (size_t i = 0; i < nbs * 64; ++i)
        if (srcf[i] >= gs || usrcf[i] >= gs) return -1;
    std::vector<uint32_t> ft, gt;
    if (pack(v, tf, tg, ft, gt)) return -1;
    const void *k = op_pick(kind, isg, nsets, kind == K_FF ? (dl ? 1 : 0) : (sl ? 1 : 0), kind == K_FF ? (cdl ? 1 : 0) : (dl ? 1 : 0), lt != 0);
    if (!k) return -1;
    int rc;
    if ((rc = no_static_lds(k))) return rc;

    OpArgs a;
    std::memset(&a, 0, sizeof a);
    MOp &op = a.op;
    op.type = isg ? qpd::OP_G : qpd::OP_F;
    op.flags = (sl ? qpd::MF_SRC_LDS : 0) | (dl ? qpd::MF_DST_LDS : 0) | (ul ? qpd::MF_U_LDS : 0);
    if (kind == K_CHAN) op.flags |= qpd::MF_CHAN;
    if (kind == K_FGP && pre) op.flags |= qpd::MF_PRE;
    if (kind == K_GSEL) op.flags |= qpd::MF_PRE | qpd::MF_GSEL;
    if (kind == K_FF) op.flags |= qpd::MF_FF | (cdl ? qpd::MF_FF_DL : 0);
    op.d = 1;
    op.cnt = cnt;
    op.src_row = rows[0];
    op.dst_row = rows[1];
    op.u_row = rows[2];
    op.r_row = rows[3];
    op.sh_src = 4;
    op.sh_u = 8;
    op.sh_dst = 8;
    op.pad1 = 12;
    a.v = v;
    a.in_vec = in_vec ? 1 : 0;
    a.gs = gs;
    a.lds_rows = lds_rows;
    a.glb_rows = glb_rows;
    a.ystride = ystride;
    const size_t gwords = nbs * glb_rows * 64, lwords = (size_t)nblocks * nrow, ywords = nbs * (64 / gs) * ystride;
    const std::vector<uint32_t> lds0(lds, lds + lwords), slab0(slab, slab + gwords);
    DevBuf dft, dgt, dy, dli, dlo, dsl, dsf, duf, derr, dok;
    hipError_t e;
    if ((rc = upload(dft, ft.data(), 64 * 4))) return rc;
    if ((rc = upload(dgt, gt.data(), 64 * 4))) return rc;
    if ((rc = upload(dy, y, ywords * 4))) return rc;
    if ((rc = upload(dli, lds, lwords * 4))) return rc;
    if ((rc = alloc_fill(dlo, lwords * 4, 0xEE))) return rc;
    if ((rc = upload(dsl, slab, gwords * 4))) return rc;
    if ((rc = upload(dsf, srcf, nbs * 64))) return rc;
    if ((rc = upload(duf, usrcf, nbs * 64))) return rc;
    if ((rc = alloc_fill(derr, (size_t)nblocks * 4, 0))) return rc;
    if ((rc = alloc_fill(dok, (size_t)nblocks * 4, 0))) return rc;
    a.ft = (const uint32_t *)dft.p;
    a.gt = (const uint32_t *)dgt.p;
    a.y = (const int32_t *)dy.p;
    a.lds_in = (const uint32_t *)dli.p;
    a.lds_out = (uint32_t *)dlo.p;
    a.slab = (uint32_t *)dsl.p;
    a.srcf = (const uint8_t *)dsf.p;
    a.usrcf = (const uint8_t *)duf.p;
    a.err = (int32_t *)derr.p;
    a.ok = (int32_t *)dok.p;
    void *args[] = {&a};
    LK_TRY(hipLaunchKernel(k, dim3(nblocks), dim3(64), args, (kRowsAt + kCanary + nrow) * 4, nullptr));
    LK_TRY(hipDeviceSynchronize());
    LK_TRY(hipMemcpy(lds, dlo.p, lwords * 4, hipMemcpyDeviceToHost));
    LK_TRY(hipMemcpy(slab, dsl.p, gwords * 4, hipMemcpyDeviceToHost));
    LK_TRY(hipMemcpy(err, derr.p, (size_t)nblocks * 4, hipMemcpyDeviceToHost));
    LK_TRY(hipMemcpy(ok, dok.p, (size_t)nblocks * 4, hipMemcpyDeviceToHost));
    for (int b = 0; b < nblocks; ++b) {  // bit 1: the rows the op reads are what was loaded
        bool same = true;
        for (const Span &s : reads) {
            const size_t per = (size_t)nsets * 64, at = ((size_t)b * (s.lds ? lds_rows : glb_rows) + s.row) * per;
            const uint32_t *now = (s.lds ? lds : slab) + at, *was = (s.lds ? lds0.data() : slab0.data()) + at;
            same = same && std::memcmp(now, was, s.rows * per * 4) == 0;
        }
        ok[b] |= same ? 2 : 0;
    }
    return 0;
}

// root_pre_kernel<int32_t> (u8 = 0) or <uint8_t> on B frames of N = 2^n symbols, `grid` blocks of 256.
// in: in_off + B * N elements, the frames from element in_off on (in_vec: in_off keeps the rows 16- /
// 8-byte aligned).  pre: (B + 1) * N / 4 words, in (the caller's sentinels) and out.
int qpd_lk_root_pre(int u8, int n, int v, int64_t B, int grid, int in_vec, int in_off, const uint8_t *tf, const uint8_t *tg,
                    const void *in, uint32_t *pre, int32_t *err) {
    if (n < 4 || n > 12 || B < 1 || (B << (n - 4)) > (1 << 20) || grid < 1 || grid > 64 || in_off < 0 || in_off > 64) return -1;
    if (!in || !pre || !err) return -1;
    if (in_vec && (in_off & (u8 ? 7 : 3))) return -1;
    std::vector<uint32_t> ft, gt;
    if (pack(v, tf, tg, ft, gt)) return -1;
    const int N = 1 << n;
    const size_t esz = u8 ? 1 : 4, nin = (size_t)in_off + (size_t)B * N, npre = (size_t)(B + 1) * (N / 4);
    DevBuf dft, dgt, din, dpre, derr;
    int rc;
    hipError_t e;
    if ((rc = upload(dft, ft.data(), 64 * 4))) return rc;
    if ((rc = upload(dgt, gt.data(), 64 * 4))) return rc;
    if ((rc = upload(din, in, nin * esz))) return rc;
    if ((rc = upload(dpre, pre, npre * 4))) return rc;
    if ((rc = alloc_fill(derr, 4, 0))) return rc;
    FastPlan P{};
    P.N = N;
    P.n = n;
    P.v = v;
    P.in_vec = in_vec ? 1 : 0;
    P.f_tab = (const uint32_t *)dft.p;
    P.g_tab = (const uint32_t *)dgt.p;
    P.err = (int32_t *)derr.p;
    if (u8)
        qpd::root_pre_kernel<uint8_t><<<dim3(grid), dim3(256)>>>(P, (const uint8_t *)din.p + in_off, B, (uint32_t *)dpre.p);
    else
        qpd::root_pre_kernel<int32_t><<<dim3(grid), dim3(256)>>>(P, (const int32_t *)din.p + in_off, B, (uint32_t *)dpre.p);
    LK_TRY(hipGetLastError());
    LK_TRY(hipDeviceSynchronize());
    LK_TRY(hipMemcpy(pre, dpre.p, npre * 4, hipMemcpyDeviceToHost));
    LK_TRY(hipMemcpy(err, derr.p, 4, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
