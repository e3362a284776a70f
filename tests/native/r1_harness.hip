// Device harness of the fast engine's rate-1 (R1) nodes: two small kernels that call
// the real device functions of qpd_fast_special.hpp -- r1_prep (the argsort: packed min
// trees, partition_prefix_masked with its heap-sort fallback, the GEN sort_small_prefix
// path, R1PrepT packing) and r1_small<LM> / r1_multi (the survivor layers with their
// identity early-out) -- on symbols, rank tables, quanta and path metrics the caller
// chooses per lane.  One wave per block, as the decode kernel.  The harness builds the
// FastPlan (v, vcl, r1_rank), one MOp per block, a Mem whose rows all lie in LDS and
// path pointer words that make every lane read its own column.
//
// LDS of a block (words; rows of 64, the sets' rows interleaved as Mem::rw does):
//   [canary 64] [rows 0..3: source symbols | row 4: destination] x NS
//   [u_row = 5: the 16-row argsort tail (LdsSeq16, row stride 64 words)]
//   [selection scratch: NS * kSelInts] [canary 64]
// Every run reports, per block, that both canary rows are intact and that the source
// rows of every set still hold what was loaded (no set's argsort or layers may touch
// another set's symbols, nor its own).
//
// The references are plain host C++ in this library, written from the operation's
// definition: std::sort on an index array with a keys-only comparison (the argsort;
// mink on [keeps | flips]), m fork layers, bits = hard decisions XOR flips.  They use
// neither qpd_host.hpp nor stl_sort.hpp.
//
// A checker, not a stress tool: every entry point validates its arguments before any
// launch and returns -1 for what the decode kernels could not run.
#include "qpd_fast_special.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#ifndef QPD_R1_BUILD_ID
#define QPD_R1_BUILD_ID "unstamped"
#endif

namespace {

using qpd::FastPlan;
using qpd::Mem;
using qpd::MOp;

enum Inst { I_GEN7 = 0, I_RK7 = 1, I_GEN15 = 2, I_COUNT };  // r1_prep<false, GEN, MAXM>
enum Src { S_RK = 0, S_VUNI = 1, S_TAB = 2, S_COUNT };       // the rank source
enum Mode {
    M_SMALL0 = 0,   // r1_small<0>: L = 1..8, the generic selection
    M_SMALL8 = 1,   // r1_small<8>: L = 8 (the R1L instantiations' special_op)
    M_SMALL16 = 2,  // r1_small<16>: L = 9..16
    M_MULTI = 3,    // r1_multi<false, false, NS>: L = 8, ranks in the op record
    M_MULTI_GEN = 4,  // r1_multi<false, true, NS>: L = 8, any rank source
    M_COUNT
};

constexpr int kCanary = 64;
constexpr uint32_t kCanaryWord = 0xC0DE5E1Fu;
constexpr uint32_t kFillWord = 0xAAAAAAAAu;
constexpr int kSrcRows = 4, kDstRow = 4, kURow = 5, kTailRows = 16;
constexpr int kOrd = 16;  // order / symbol outputs per lane (entries q >= m: -1)

template <int NS>
struct Lay {
    static constexpr int rows = kCanary;                      // the sets' row 0 (lds_wave)
    static constexpr int tail = rows + kURow * NS * 64;       // lds_wave + Mem::rw(u_row)
    static constexpr int sel = tail + kTailRows * 64;         // the selection scratch
    static constexpr int back = sel + NS * qpd::kSelInts;     // the second canary row
    static constexpr int total = back + kCanary;
};

// src: [block][set][4][64] symbol words.
template <int NS>
__device__ __forceinline__ void lds_fill(uint32_t *lds, const uint32_t *__restrict__ src, int lane) {
    lds[lane] = kCanaryWord ^ (uint32_t)lane;
    lds[Lay<NS>::back + lane] = ~kCanaryWord ^ (uint32_t)lane;
    for (int i = lane; i < Lay<NS>::back - kCanary; i += 64) lds[kCanary + i] = kFillWord;
    __syncthreads();
    for (int s = 0; s < NS; ++s)
        for (int w = 0; w < kSrcRows; ++w)
            lds[Lay<NS>::rows + (w * NS + s) * 64 + lane] = src[(((size_t)blockIdx.x * NS + s) * kSrcRows + w) * 64 + lane];
    __syncthreads();
}

// bit 0: the canaries are intact; bit 1: every set's source rows are unchanged.
template <int NS>
__device__ __forceinline__ void lds_verify(const uint32_t *lds, const uint32_t *__restrict__ src, int lane, int32_t *ok) {
    __syncthreads();
    const bool can = lds[lane] == (kCanaryWord ^ (uint32_t)lane) && lds[Lay<NS>::back + lane] == (~kCanaryWord ^ (uint32_t)lane);
    bool same = true;
    for (int s = 0; s < NS; ++s)
        for (int w = 0; w < kSrcRows; ++w)
            same = same && lds[Lay<NS>::rows + (w * NS + s) * 64 + lane] == src[(((size_t)blockIdx.x * NS + s) * kSrcRows + w) * 64 + lane];
    const uint64_t bc = __builtin_amdgcn_ballot_w64(!can), bs = __builtin_amdgcn_ballot_w64(!same);
    if (lane == 0) ok[blockIdx.x] = (bc == 0 ? 1 : 0) | (bs == 0 ? 2 : 0);
}

template <int NS>
__device__ __forceinline__ Mem mem_of(uint32_t *lds_wave) {
    Mem M;
    M.lds = lds_wave;
    M.gp = nullptr;
    M.rs = __builtin_amdgcn_make_buffer_rsrc((void *)nullptr, 0, 0, 0x00020000);  // no slab: every row is in LDS
    M.so = 0;
    M.ns = NS;
    return M;
}

__device__ __forceinline__ uint64_t self_fields(int gl) {  // every pointer field = the lane's own slot
    uint64_t self = 0;
    for (int d = 0; d < 16; ++d) self |= (uint64_t)gl << (4 * d);
    return self;
}

template <bool GEN, int MAXM, int NS>
__global__ __launch_bounds__(64) void argsort_kernel(const MOp *__restrict__ ops, const double *__restrict__ vcl,
                                                     const uint16_t *__restrict__ rk, int v, int L, int gs,
                                                     const uint32_t *__restrict__ src, int32_t *__restrict__ ord,
                                                     int32_t *__restrict__ sym, uint32_t *__restrict__ hw,
                                                     int32_t *__restrict__ ok) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[Lay<NS>::total];
    const int lane = threadIdx.x, gl = lane & (gs - 1), gbase = lane - gl;
    lds_fill<NS>(lds, src, lane);
    uint32_t *const lds_wave = lds + Lay<NS>::rows;
    FastPlan P{};
    P.v = v;
    P.vcl = vcl;
    P.r1_rank = rk;
    const Mem M0 = mem_of<NS>(lds_wave);
    const MOp op = ops[blockIdx.x];
    const int temp = op.cnt, m = (L - 1) < temp ? (L - 1) : temp;
    qpd::PathT<false> st;
    st.pm = 0.0;
    st.ps = st.pu = self_fields(gl);
#pragma unroll 1
    for (int s = 0; s < NS; ++s) {  // the sets one after the other in the one tail, as r1_multi
        const qpd::R1PrepT<MAXM> r = qpd::r1_prep<false, GEN, MAXM>(P, M0.set(s), op, st, gbase, L, lane, temp, lds_wave);
        const size_t at = ((size_t)blockIdx.x * NS + s) * 64 + lane;
        for (int q = 0; q < kOrd; ++q) {
            const bool in = q < m && q < MAXM;
            ord[at * kOrd + q] = in ? r.ord(q < MAXM ? q : 0) : -1;
            sym[at * kOrd + q] = in ? (int32_t)r.sym(q < MAXM ? q : 0) : -1;
        }
        hw[at] = r.hw;
    }
    lds_verify<NS>(lds, src, lane, ok);
}

template <int MODE, int NS>
__global__ __launch_bounds__(64) void node_kernel(const MOp *__restrict__ ops, const double *__restrict__ vcl,
                                                  const uint16_t *__restrict__ rk, int v, int L, int gs,
                                                  const uint32_t *__restrict__ src, const double *__restrict__ pm_in,
                                                  uint32_t *__restrict__ word, double *__restrict__ pm_out,
                                                  int32_t *__restrict__ lineage, int32_t *__restrict__ ok) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[Lay<NS>::total];
    const int lane = threadIdx.x, gl = lane & (gs - 1), gbase = lane - gl;
    lds_fill<NS>(lds, src, lane);
    uint32_t *const lds_wave = lds + Lay<NS>::rows;
    int *const sel_all = (int *)(lds + Lay<NS>::sel);
    const int sstride = 64;
    FastPlan P{};
    P.v = v;
    P.vcl = vcl;
    P.r1_rank = rk;
    Mem Mv[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) Mv[s] = mem_of<NS>(lds_wave).set(s);
    const MOp op = ops[blockIdx.x];
    qpd::PathT<false> st[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        st[s].pm = pm_in[((size_t)blockIdx.x * NS + s) * 64 + lane];
        st[s].ps = st[s].pu = self_fields(gl);
    }
    if constexpr (MODE == M_MULTI || MODE == M_MULTI_GEN) {
        qpd::r1_multi<false, MODE == M_MULTI_GEN, NS>(P, Mv, op, st, sel_all, sstride, gl, gbase, lane, lds_wave, 0u, nullptr);
    } else {
        constexpr int LM = MODE == M_SMALL8 ? 8 : MODE == M_SMALL16 ? 16 : 0;
#pragma unroll
        for (int s = 0; s < NS; ++s)  // as special_op runs the sets: one after the other
            qpd::r1_small<LM>(P, Mv[s], op, st[s], sel_all + sstride * s, NS * sstride, gl, gbase, L, lane, op.cnt, lds_wave);
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const size_t at = ((size_t)blockIdx.x * NS + s) * 64 + lane;
        word[at] = lds_wave[(kDstRow * NS + s) * 64 + lane];
        pm_out[at] = st[s].pm;
        lineage[at] = qpd::pfield(st[s].ps, 8);  // a field no op of the node writes: the slot it started in
    }
    lds_verify<NS>(lds, src, lane, ok);
}

int group_size(int L) {
    if (L < 1 || L > 16) return 0;
    if (L > 8) return 16;
    int g = 1;
    while (g < L) g <<= 1;
    return g;
}

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

#define R1_TRY(x) \
    if ((e = (x)) != hipSuccess) return (int)e

int upload(DevBuf &d, const void *h, size_t bytes) {
    hipError_t e;
    R1_TRY(hipMalloc(&d.p, bytes ? bytes : 1));
    if (bytes) R1_TRY(hipMemcpy(d.p, h, bytes, hipMemcpyHostToDevice));
    return 0;
}

int alloc_fill(DevBuf &d, size_t bytes, int fill) {
    hipError_t e;
    R1_TRY(hipMalloc(&d.p, bytes ? bytes : 1));
    R1_TRY(hipMemset(d.p, fill, bytes ? bytes : 1));
    return 0;
}

// [block][set][64][temp] symbols -> [block][set][4][64] words (symbol j in nibble j % 8 of word j / 8)
std::vector<uint32_t> pack_symbols(const uint8_t *sym, size_t nbs, int temp) {
    std::vector<uint32_t> w(nbs * kSrcRows * 64, 0u);
    for (size_t bs = 0; bs < nbs; ++bs)
        for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < temp; ++j)
                w[(bs * kSrcRows + (j >> 3)) * 64 + lane] |= (uint32_t)sym[(bs * 64 + lane) * temp + j] << (4 * (j & 7));
    return w;
}

bool symbols_ok(const uint8_t *sym, size_t n, int v) {
    for (size_t i = 0; i < n; ++i)
        if (sym[i] >= v) return false;
    return true;
}

// The op record of one block's node.  row: [v] rank << 1 | sign of the node's one rank row (S_RK).
MOp make_op(int src_mode, int temp, int tab, int vrow, const uint16_t *row, int v) {
    MOp op;
    std::memset(&op, 0, sizeof op);
    op.type = qpd::OP_R1;
    op.flags = qpd::MF_SRC_LDS | qpd::MF_DST_LDS | (temp > qpd::stl::kThreshold ? qpd::MF_R1_LDS : 0);
    op.d = 1;
    op.cnt = temp;
    op.src_row = 0;
    op.dst_row = kDstRow;
    op.u_row = kURow;
    op.sh_src = 4;
    op.sh_u = 8;
    op.sh_dst = 4;
    op.tab = tab;
    op.vrow = vrow;
    if (src_mode == S_RK || src_mode == S_VUNI) op.flags |= qpd::MF_VUNI;
    if (src_mode == S_RK) {
        uint64_t rk = 0;
        uint32_t sg = 0;
        for (int sy = 0; sy < v; ++sy) {
            rk |= (uint64_t)(row[sy] >> 1) << (4 * sy);
            sg |= (uint32_t)(row[sy] & 1) << sy;
        }
        op.flags |= qpd::MF_R1_RK;
        op.r_row = (int32_t)(uint32_t)rk;
        op.tab2 = (int32_t)(uint32_t)(rk >> 32);
        op.pad1 = (int32_t)sg;
    }
    return op;
}

// [temp][v] rank table of one node: what the rank source can carry.
bool table_ok(int src_mode, const uint16_t *t, int temp, int v) {
    for (int j = 0; j < temp; ++j)
        for (int sy = 0; sy < v; ++sy) {
            const int e = t[j * v + sy];
            if ((e >> 1) >= (src_mode == S_RK ? 16 : 2047)) return false;  // rank << 5 | element in 16 bits, below 0xFFFF
            if (src_mode != S_TAB && e != t[sy]) return false;           // one rank row
        }
    return true;
}

// --- host references -----------------------------------------------------------------

// argsort: std::sort on the index array, keys-only comparison
template <class K>
void argsort_ref(const K *key, int n, int *idx) {
    for (int i = 0; i < n; ++i) idx[i] = i;
    std::sort(idx, idx + n, [&](int a, int b) { return key[a] < key[b]; });
}

// libstdc++'s introsort partition loop on entries compared by rank alone, followed as far as
// it can reach the first m outputs: does it arrive at the depth limit, after how many partitions?
void median_to_first(int *e, int result, int a, int b, int c) {
    int pick;
    if (e[a] < e[b]) pick = e[b] < e[c] ? b : e[a] < e[c] ? c : a;
    else pick = e[a] < e[c] ? a : e[b] < e[c] ? c : b;
    std::swap(e[result], e[pick]);
}

int hoare_partition(int *e, int first, int last, int pivot) {
    for (;;) {
        while (e[first] < e[pivot]) ++first;
        --last;
        while (e[pivot] < e[last]) --last;
        if (!(first < last)) return first;
        std::swap(e[first], e[last]);
        ++first;
    }
}

bool reaches_depth_limit(const int *rank, int n, int m, int *parts) {
    std::vector<int> e(rank, rank + n);  // keys only: the elements' identities do not steer the partitions
    int f = 0, l = n, dl = 0, end = n;
    for (int t = n; t > 1; t >>= 1) dl += 2;
    *parts = 0;
    while (l - f > 16) {
        if (dl == 0) return true;
        --dl;
        ++*parts;
        median_to_first(e.data(), f, f + 1, f + (l - f) / 2, l - 1);
        const int cut = hoare_partition(e.data(), f + 1, l, f);
        if (cut >= m && cut < end) end = cut;
        if (l - cut > 16) {
            if (cut >= end) break;
            f = cut;
        } else {
            l = cut;
        }
    }
    return false;
}

// [v] quanta -> rank << 1 | sign (dense ranks of the magnitudes; equal magnitudes, equal ranks)
void rank_row(const double *q, int v, uint16_t *out) {
    std::vector<double> mags(q, q + v);
    for (double &x : mags) x = std::fabs(x);
    std::sort(mags.begin(), mags.end());
    mags.erase(std::unique(mags.begin(), mags.end()), mags.end());
    for (int sy = 0; sy < v; ++sy) {
        const int r = (int)(std::lower_bound(mags.begin(), mags.end(), std::fabs(q[sy])) - mags.begin());
        out[sy] = (uint16_t)((r << 1) | (q[sy] < 0 ? 1 : 0));
    }
}

}  // namespace

extern "C" {

const char *qpd_r1_build_id() {
    static const char tag[] = "qpd-r1h-build-id:" QPD_R1_BUILD_ID;
    return tag + 17;
}

int qpd_r1_group_size(int L) { return group_size(L); }

// r1_prep instantiation `inst` on nblocks one-wave blocks of nsets frame sets.
// table: [nblocks][temp][v] rank << 1 | sign; sym: [nblocks][nsets][64][temp];
// ord, symo: [nblocks][nsets][64][16] (-1 from m on); hw: [nblocks][nsets][64]; ok: [nblocks].
// Returns the HIP error code, or -1 for arguments the kernels cannot run (nothing launched).
int qpd_r1_argsort(int inst, int src_mode, int L, int temp, int v, int nsets, int nblocks, const uint16_t *table,
                   const uint8_t *sym, int32_t *ord, int32_t *symo, uint32_t *hw, int32_t *ok) {
    const int gs = group_size(L);
    if (inst < 0 || inst >= I_COUNT || src_mode < 0 || src_mode >= S_COUNT) return -1;
    if (gs == 0 || temp < 1 || temp > 32 || v < 1 || v > 16 || nsets < 1 || nsets > 2) return -1;
    if (nblocks < 1 || nblocks > (1 << 16)) return -1;
    if (!table || !sym || !ord || !symo || !hw || !ok) return -1;
    const int maxm = inst == I_GEN15 ? 15 : qpd::kMaxM, m = std::min(L - 1, temp);
    if (m > maxm) return -1;
    if (inst == I_RK7 && src_mode != S_RK) return -1;  // GEN = false: ranks in the op record only
    const size_t nbs = (size_t)nblocks * nsets, n = nbs * 64;
    if (!symbols_ok(sym, n * temp, v)) return -1;
    std::vector<MOp> ops(nblocks);
    for (int b = 0; b < nblocks; ++b) {
        const uint16_t *t = table + (size_t)b * temp * v;
        if (!table_ok(src_mode, t, temp, v)) return -1;
        ops[b] = make_op(src_mode, temp, b * temp * v, 0, t, v);
    }
    const std::vector<uint32_t> words = pack_symbols(sym, nbs, temp);
    const std::vector<double> vcl(32 * 16, 1.0);  // r1_prep reads no quanta
    DevBuf dop, dv, dt, dw, dord, dsym, dhw, dok;
    int rc;
    hipError_t e;
    if ((rc = upload(dop, ops.data(), ops.size() * sizeof(MOp)))) return rc;
    if ((rc = upload(dv, vcl.data(), vcl.size() * sizeof(double)))) return rc;
    if ((rc = upload(dt, table, (size_t)nblocks * temp * v * sizeof(uint16_t)))) return rc;
    if ((rc = upload(dw, words.data(), words.size() * sizeof(uint32_t)))) return rc;
    if ((rc = alloc_fill(dord, n * kOrd * sizeof(int32_t), 0xEE))) return rc;
    if ((rc = alloc_fill(dsym, n * kOrd * sizeof(int32_t), 0xEE))) return rc;
    if ((rc = alloc_fill(dhw, n * sizeof(uint32_t), 0xEE))) return rc;
    if ((rc = alloc_fill(dok, (size_t)nblocks * sizeof(int32_t), 0))) return rc;
    const void *fn;
#define R1_PICK(GEN, MAXM)                                                                          \
    (nsets == 2 ? reinterpret_cast<const void *>(&argsort_kernel<GEN, MAXM, 2>)                     \
                : reinterpret_cast<const void *>(&argsort_kernel<GEN, MAXM, 1>))
    fn = inst == I_GEN7 ? R1_PICK(true, qpd::kMaxM) : inst == I_RK7 ? R1_PICK(false, qpd::kMaxM) : R1_PICK(true, 15);
#undef R1_PICK
    const MOp *aop = (const MOp *)dop.p;
    const double *av = (const double *)dv.p;
    const uint16_t *at = (const uint16_t *)dt.p;
    const uint32_t *aw = (const uint32_t *)dw.p;
    int32_t *ao = (int32_t *)dord.p, *as = (int32_t *)dsym.p, *ak = (int32_t *)dok.p;
    uint32_t *ah = (uint32_t *)dhw.p;
    int avv = v, aL = L, ags = gs;
    void *args[] = {&aop, &av, &at, &avv, &aL, &ags, &aw, &ao, &as, &ah, &ak};
    R1_TRY(hipLaunchKernel(fn, dim3(nblocks), dim3(64), args, 0, nullptr));
    R1_TRY(hipDeviceSynchronize());
    R1_TRY(hipMemcpy(ord, dord.p, n * kOrd * sizeof(int32_t), hipMemcpyDeviceToHost));
    R1_TRY(hipMemcpy(symo, dsym.p, n * kOrd * sizeof(int32_t), hipMemcpyDeviceToHost));
    R1_TRY(hipMemcpy(hw, dhw.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    R1_TRY(hipMemcpy(ok, dok.p, (size_t)nblocks * sizeof(int32_t), hipMemcpyDeviceToHost));
    return 0;
}

// The argsort's reference, same shapes: per lane, std::sort on the indices 0..temp-1 by
// rank[a] < rank[b] (keys only), first m = min(L - 1, temp) outputs with their symbols;
// hw bit j = the sign bit of element j's table entry.
int qpd_r1_argsort_ref(int L, int temp, int v, int nsets, int nblocks, const uint16_t *table, const uint8_t *sym,
                       int32_t *ord, int32_t *symo, uint32_t *hw) {
    if (L < 1 || L > 16 || temp < 1 || temp > 32 || v < 1 || v > 16 || nsets < 1 || nsets > 2 || nblocks < 1) return -1;
    const int m = std::min(L - 1, temp);
    int rank[32], idx[32];
    for (int b = 0; b < nblocks; ++b)
        for (int sl = 0; sl < nsets * 64; ++sl) {
            const size_t at = (size_t)b * nsets * 64 + sl;
            const uint8_t *sy = sym + at * temp;
            uint32_t h = 0;
            for (int j = 0; j < temp; ++j) {
                if (sy[j] >= v) return -1;
                const int e = table[((size_t)b * temp + j) * v + sy[j]];
                rank[j] = e >> 1;
                h |= (uint32_t)(e & 1) << j;
            }
            argsort_ref(rank, temp, idx);
            for (int q = 0; q < kOrd; ++q) {
                ord[at * kOrd + q] = q < m ? idx[q] : -1;
                symo[at * kOrd + q] = q < m ? sy[idx[q]] : -1;
            }
            hw[at] = h;
        }
    return 0;
}

// Does the introsort of rank array i ([n][temp] ranks) reach its depth limit -- the heap-sort
// fallback of partition_prefix_masked -- when the first m outputs are wanted, and how many
// partitions does it run?  (temp <= 16: no partitions, never.)
int qpd_r1_heap(int temp, int m, int64_t n, const int32_t *ranks, uint8_t *fell, int32_t *parts) {
    if (temp < 1 || temp > 32 || m < 0 || m > temp || n < 0 || !ranks || !fell || !parts) return -1;
    for (int64_t i = 0; i < n; ++i) {
        int p = 0;
        fell[i] = reaches_depth_limit(ranks + i * temp, temp, m, &p) ? 1 : 0;
        parts[i] = p;
    }
    return 0;
}

// A whole R1 node.  quanta: [nblocks][v] (the node's one quanta row); pm: [nblocks][nsets][64]
// path metrics (the lanes gl >= L of a group are padding: they run as +inf); sym as above.
// word, pm_out, lineage: [nblocks][nsets][64]; ok: [nblocks].
int qpd_r1_node(int mode, int src_mode, int L, int temp, int v, int nsets, int nblocks, const double *quanta,
                const double *pm, const uint8_t *sym, uint32_t *word, double *pm_out, int32_t *lineage, int32_t *ok) {
    const int gs = group_size(L);
    if (mode < 0 || mode >= M_COUNT || src_mode < 0 || src_mode >= S_COUNT) return -1;
    if (gs == 0 || temp < 1 || temp > 32 || v < 1 || v > 16 || nsets < 1 || nsets > 2) return -1;
    if (nblocks < 1 || nblocks > (1 << 16)) return -1;
    if (!quanta || !pm || !sym || !word || !pm_out || !lineage || !ok) return -1;
    if (mode == M_SMALL0 && L > 8) return -1;
    if ((mode == M_SMALL8 || mode == M_MULTI || mode == M_MULTI_GEN) && L != 8) return -1;
    if (mode == M_SMALL16 && L < 9) return -1;
    if (mode == M_MULTI && src_mode != S_RK) return -1;
    const size_t nbs = (size_t)nblocks * nsets, n = nbs * 64;
    if (!symbols_ok(sym, n * temp, v)) return -1;
    for (size_t i = 0; i < (size_t)nblocks * v; ++i)
        if (!std::isfinite(quanta[i])) return -1;
    std::vector<double> pmv(pm, pm + n);
    for (size_t i = 0; i < n; ++i) {
        if ((int)(i & (gs - 1)) >= L) pmv[i] = HUGE_VAL;
        if (!(pmv[i] >= 0.0)) return -1;  // metrics are >= +0 or +inf, never NaN
    }
    // per block: the quanta row and its rank row, once per element (the per-element sources read row j)
    std::vector<MOp> ops(nblocks);
    std::vector<double> vcl((size_t)nblocks * 32 * v);
    std::vector<uint16_t> tab((size_t)nblocks * 32 * v);
    for (int b = 0; b < nblocks; ++b) {
        uint16_t row[16];
        rank_row(quanta + (size_t)b * v, v, row);
        for (int j = 0; j < 32; ++j)
            for (int sy = 0; sy < v; ++sy) {
                vcl[((size_t)b * 32 + j) * v + sy] = quanta[(size_t)b * v + sy];
                tab[((size_t)b * 32 + j) * v + sy] = row[sy];
            }
        ops[b] = make_op(src_mode, temp, b * 32 * v, b * 32, row, v);
    }
    const std::vector<uint32_t> words = pack_symbols(sym, nbs, temp);
    DevBuf dop, dv, dt, dw, dpm, dwo, dpo, dli, dok;
    int rc;
    hipError_t e;
    if ((rc = upload(dop, ops.data(), ops.size() * sizeof(MOp)))) return rc;
    if ((rc = upload(dv, vcl.data(), vcl.size() * sizeof(double)))) return rc;
    if ((rc = upload(dt, tab.data(), tab.size() * sizeof(uint16_t)))) return rc;
    if ((rc = upload(dw, words.data(), words.size() * sizeof(uint32_t)))) return rc;
    if ((rc = upload(dpm, pmv.data(), n * sizeof(double)))) return rc;
    if ((rc = alloc_fill(dwo, n * sizeof(uint32_t), 0xEE))) return rc;
    if ((rc = alloc_fill(dpo, n * sizeof(double), 0xEE))) return rc;
    if ((rc = alloc_fill(dli, n * sizeof(int32_t), 0xEE))) return rc;
    if ((rc = alloc_fill(dok, (size_t)nblocks * sizeof(int32_t), 0))) return rc;
#define R1_PICK(MODE)                                                                      \
    (nsets == 2 ? reinterpret_cast<const void *>(&node_kernel<MODE, 2>)                    \
                : reinterpret_cast<const void *>(&node_kernel<MODE, 1>))
    const void *fn = mode == M_SMALL0    ? R1_PICK(M_SMALL0)
                     : mode == M_SMALL8  ? R1_PICK(M_SMALL8)
                     : mode == M_SMALL16 ? R1_PICK(M_SMALL16)
                     : mode == M_MULTI   ? R1_PICK(M_MULTI)
                                         : R1_PICK(M_MULTI_GEN);
#undef R1_PICK
    const MOp *aop = (const MOp *)dop.p;
    const double *av = (const double *)dv.p, *apm = (const double *)dpm.p;
    const uint16_t *at = (const uint16_t *)dt.p;
    const uint32_t *aw = (const uint32_t *)dw.p;
    uint32_t *awo = (uint32_t *)dwo.p;
    double *apo = (double *)dpo.p;
    int32_t *ali = (int32_t *)dli.p, *ak = (int32_t *)dok.p;
    int avv = v, aL = L, ags = gs;
    void *args[] = {&aop, &av, &at, &avv, &aL, &ags, &aw, &apm, &awo, &apo, &ali, &ak};
    R1_TRY(hipLaunchKernel(fn, dim3(nblocks), dim3(64), args, 0, nullptr));
    R1_TRY(hipDeviceSynchronize());
    R1_TRY(hipMemcpy(word, dwo.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    R1_TRY(hipMemcpy(pm_out, dpo.p, n * sizeof(double), hipMemcpyDeviceToHost));
    R1_TRY(hipMemcpy(lineage, dli.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    R1_TRY(hipMemcpy(ok, dok.p, (size_t)nblocks * sizeof(int32_t), hipMemcpyDeviceToHost));
    return 0;
}

// The node's reference, from its definition, per lane group of gs = qpd_r1_group_size(L) lanes:
// path i (i < L) holds the llrs quanta[sym_i[j]], its hard decisions (llr < 0) and the argsort of
// its |llr| (above).  Each of the m = min(L - 1, temp) layers offers, for the path in slot i,
// keep (metric pm_i) and flip of its lineage's next position in argsort order (pm_i + |llr| there);
// mink -- std::sort on the 2L candidate indices by key, first L -- names the survivors, slot t
// taking its candidate's metric and lineage and, for a flip, a position toggled: the one slot t
// itself offered before the selection, not its parent's (the reference decoder's flip-index
// quirk, SURVEY.md H2, which every engine reproduces).  Bits = the lineage's hard decisions XOR
// the flips.  ident: bit q set where layer q's selection was the
// identity (slot t keeps candidate t, for every t < L); the same word in every lane of a group.
int qpd_r1_node_ref(int L, int temp, int v, int nsets, int nblocks, const double *quanta, const double *pm,
                    const uint8_t *sym, uint32_t *word, double *pm_out, int32_t *lineage, uint32_t *ident) {
    const int gs = group_size(L);
    if (gs == 0 || temp < 1 || temp > 32 || v < 1 || v > 16 || nsets < 1 || nsets > 2 || nblocks < 1) return -1;
    const int m = std::min(L - 1, temp);
    const uint32_t mask = temp < 32 ? (1u << temp) - 1u : 0xffffffffu;
    std::vector<double> mag(L * 32), key(2 * L), npm(L), cpm(L);
    std::vector<int> ord(L * 32), idx(2 * L), origin(L), norigin(L);
    std::vector<uint32_t> hard(L), flips(L), nflips(L);
    for (int b = 0; b < nblocks; ++b)
        for (int s = 0; s < nsets; ++s)
            for (int g = 0; g < 64; g += gs) {
                const size_t at = ((size_t)b * nsets + s) * 64 + g;
                for (int i = 0; i < L; ++i) {
                    hard[i] = 0;
                    for (int j = 0; j < temp; ++j) {
                        const int sy = sym[(at + i) * temp + j];
                        if (sy >= v) return -1;
                        const double l = quanta[(size_t)b * v + sy];
                        mag[i * 32 + j] = std::fabs(l);
                        hard[i] |= (uint32_t)(l < 0) << j;
                    }
                    argsort_ref(&mag[i * 32], temp, &ord[i * 32]);
                    cpm[i] = pm[at + i];
                    origin[i] = i;
                    flips[i] = 0;
                }
                uint32_t idm = 0;
                for (int q = 0; q < m; ++q) {
                    for (int i = 0; i < L; ++i) {
                        key[i] = cpm[i];
                        key[L + i] = cpm[i] + mag[origin[i] * 32 + ord[origin[i] * 32 + q]];
                    }
                    argsort_ref(key.data(), 2 * L, idx.data());
                    bool id = true;
                    for (int t = 0; t < L; ++t) {
                        const int c = idx[t], p = c < L ? c : c - L;
                        id = id && c == t;
                        npm[t] = key[c];
                        norigin[t] = origin[p];
                        nflips[t] = flips[p] ^ (c >= L ? 1u << ord[origin[t] * 32 + q] : 0u);  // H2: slot t's own position
                    }
                    idm |= (uint32_t)id << q;
                    for (int t = 0; t < L; ++t) {
                        cpm[t] = npm[t];
                        origin[t] = norigin[t];
                        flips[t] = nflips[t];
                    }
                }
                for (int i = 0; i < gs; ++i) {
                    word[at + i] = i < L ? (hard[origin[i]] ^ flips[i]) & mask : 0u;
                    pm_out[at + i] = i < L ? cpm[i] : HUGE_VAL;
                    lineage[at + i] = i < L ? origin[i] : -1;
                    ident[at + i] = idm;
                }
            }
    return 0;
}

}  // extern "C"
