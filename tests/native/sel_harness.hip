// Device harness of the list decoders' 2L -> L survivor selection: one small kernel
// that calls the selection primitives of qpd_fast_select.hpp / qpd_common.hpp directly, on
// keys the caller chooses per lane, with the LDS laid out as lut_fast_kernel lays it
// out (set s's 64 slots at sel_all + 64 * s, its junk row NS * 64 words on) between
// two rows of canary words.  tests/test_gpu_selection.py compares what it returns
// with the reference of the operation, exported from the same library: mink
// (SCLLUTDecoder.cpp:8-21) in plain host C++, std::sort on the indices 0..2L-1 by
// key[a] < key[b], first L outputs; keep i at index i, flip i at L + i.
//
// A checker, not a stress tool: the entry point refuses every L and set count the
// decode kernels cannot run (L outside 1..16, more than 2 sets) before it launches.
#include "qpd_fast_select.hpp"
#include "qpd_common.hpp"
#include "qpd_mop.hpp"  // kSelInts

#include <algorithm>
#include <vector>

#include "stl_sort.hpp"

#ifndef QPD_SEL_BUILD_ID
#define QPD_SEL_BUILD_ID "unstamped"
#endif

namespace {

enum Prim {
    P_GENERIC = 0,   // select_survivors, L = 1..8, groups of pow2 >= L
    P_SEL8 = 1,      // select_survivors8, L = 8
    P_SEL16 = 2,     // select_survivors16, L = 9..16
    P_SEL16_SER = 3, // select_survivors16<true>: the groups of the block's mask replay serially
    P_KEEP8 = 4,     // keep_all8, L = 8
    P_KEEP16 = 5,    // keep_all16, L = 9..16
    P_COUNT
};

constexpr int kCanary = 64;                 // words before and after the selection rows
constexpr uint32_t kCanaryWord = 0xC0DE5E1Fu;
constexpr uint32_t kFillWord = 0xAAAAAAAAu;  // the selection rows before the first call

// One wave per block, as the decode kernel.  keep / flip / parent / upper / ident:
// [block][set][lane]; force: [block][set] group masks (P_SEL16_SER only).
template <int PRIM, int NS>
__global__ __launch_bounds__(64) void sel_kernel(const double *__restrict__ keep, const double *__restrict__ flip,
                                                 const uint8_t *__restrict__ force, int L, int gs,
                                                 int32_t *__restrict__ parent, int32_t *__restrict__ upper,
                                                 int32_t *__restrict__ ident, int32_t *__restrict__ canary_ok) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kCanary + NS * qpd::kSelInts + kCanary];
    const int lane = threadIdx.x, gl = lane & (gs - 1), gbase = lane - gl;
    uint32_t *const tail = lds + kCanary + NS * qpd::kSelInts;
    lds[lane] = kCanaryWord ^ (uint32_t)lane;
    tail[lane] = ~kCanaryWord ^ (uint32_t)lane;
    for (int i = lane; i < NS * qpd::kSelInts; i += 64) lds[kCanary + i] = kFillWord;
    __syncthreads();
    int *const sel_all = (int *)(lds + kCanary);
    const int sstride = 64;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const size_t at = ((size_t)blockIdx.x * NS + s) * 64 + lane;
        const double kk = keep[at], kf = flip[at];
        int *const sel = sel_all + sstride * s;
        const int sj = NS * sstride;
        qpd::Sel r;
        r.parent = gl;
        r.upper = false;
        bool id = false;
        if constexpr (PRIM == P_GENERIC) r = qpd::select_survivors(kk, kf, gl, gbase, L, sel);
        else if constexpr (PRIM == P_SEL8) r = qpd::select_survivors8(kk, kf, gl, gbase, lane, sel, sj);
        else if constexpr (PRIM == P_SEL16) r = qpd::select_survivors16(kk, kf, gl, gbase, L, lane, sel, sj);
        else if constexpr (PRIM == P_SEL16_SER)
            r = qpd::select_survivors16<true>(kk, kf, gl, gbase, L, lane, sel, sj, force[(size_t)blockIdx.x * NS + s]);
        else if constexpr (PRIM == P_KEEP8)
            id = qpd::keep_all8(__builtin_bit_cast(uint64_t, kk), __builtin_bit_cast(uint64_t, kf), gl);
        else
            id = qpd::keep_all16(__builtin_bit_cast(uint64_t, kk), __builtin_bit_cast(uint64_t, kf), gl, gbase, L);
        parent[at] = r.parent;
        upper[at] = r.upper ? 1 : 0;
        ident[at] = id ? 1 : 0;
    }
    __syncthreads();
    const bool ok = lds[lane] == (kCanaryWord ^ (uint32_t)lane) && tail[lane] == (~kCanaryWord ^ (uint32_t)lane);
    const uint64_t bad = __builtin_amdgcn_ballot_w64(!ok);
    if (lane == 0) canary_ok[blockIdx.x] = bad == 0 ? 1 : 0;
}

template <int PRIM>
const void *kernel_of(int nsets) {
    return nsets == 2 ? reinterpret_cast<const void *>(&sel_kernel<PRIM, 2>)
                      : reinterpret_cast<const void *>(&sel_kernel<PRIM, 1>);
}

// The lane-group size the plan runs L at (0: L is not one the primitive serves).
int group_size(int prim, int L) {
    switch (prim) {
        case P_GENERIC: {
            if (L < 1 || L > 8) return 0;
            int g = 1;
            while (g < L) g <<= 1;
            return g;
        }
        case P_SEL8:
        case P_KEEP8: return L == 8 ? 8 : 0;
        case P_SEL16:
        case P_SEL16_SER:
        case P_KEEP16: return L >= 9 && L <= 16 ? 16 : 0;
        default: return 0;
    }
}

struct KeySeq {  // mink's index array: elements are candidate indices, compared by their keys
    int *idx;
    const double *key;
    int get(int p) { return idx[p]; }
    void set(int p, int e) { idx[p] = e; }
    bool less(int a, int b) { return key[a] < key[b]; }
};

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

}  // namespace

extern "C" {

const char *qpd_sel_build_id() {
    static const char tag[] = "qpd-sel-build-id:" QPD_SEL_BUILD_ID;
    return tag + 17;
}

int qpd_sel_group_size(int prim, int L) { return group_size(prim, L); }

// Runs primitive `prim` on nblocks one-wave blocks of nsets frame sets.  Returns the
// HIP error code, or -1 for arguments the decode kernels could not produce (nothing
// is launched then).
int qpd_sel_run(int prim, int L, int nsets, int nblocks, const double *keep, const double *flip, const uint8_t *force,
                int32_t *parent, int32_t *upper, int32_t *ident, int32_t *canary_ok) {
    const int gs = group_size(prim, L);
    if (gs == 0 || nsets < 1 || nsets > 2 || nblocks < 1 || nblocks > (1 << 20)) return -1;
    if (!keep || !flip || !parent || !upper || !ident || !canary_ok) return -1;
    if (prim == P_SEL16_SER) {
        if (!force) return -1;
        for (size_t i = 0; i < (size_t)nblocks * nsets; ++i)
            if (force[i] > 15) return -1;  // four lane groups
    }
    const size_t n = (size_t)nblocks * nsets * 64;
    DevBuf dk, df, dm, dp, du, di, dc;
    hipError_t e;
#define SEL_TRY(x) \
    if ((e = (x)) != hipSuccess) return (int)e
    SEL_TRY(hipMalloc(&dk.p, n * sizeof(double)));
    SEL_TRY(hipMalloc(&df.p, n * sizeof(double)));
    SEL_TRY(hipMalloc(&dm.p, (size_t)nblocks * nsets));
    SEL_TRY(hipMalloc(&dp.p, n * sizeof(int32_t)));
    SEL_TRY(hipMalloc(&du.p, n * sizeof(int32_t)));
    SEL_TRY(hipMalloc(&di.p, n * sizeof(int32_t)));
    SEL_TRY(hipMalloc(&dc.p, (size_t)nblocks * sizeof(int32_t)));
    SEL_TRY(hipMemcpy(dk.p, keep, n * sizeof(double), hipMemcpyHostToDevice));
    SEL_TRY(hipMemcpy(df.p, flip, n * sizeof(double), hipMemcpyHostToDevice));
    if (prim == P_SEL16_SER) SEL_TRY(hipMemcpy(dm.p, force, (size_t)nblocks * nsets, hipMemcpyHostToDevice));
    SEL_TRY(hipMemset(dp.p, 0xFF, n * sizeof(int32_t)));
    SEL_TRY(hipMemset(du.p, 0xFF, n * sizeof(int32_t)));
    SEL_TRY(hipMemset(di.p, 0xFF, n * sizeof(int32_t)));
    SEL_TRY(hipMemset(dc.p, 0, (size_t)nblocks * sizeof(int32_t)));
    const void *fn = prim == P_GENERIC     ? kernel_of<P_GENERIC>(nsets)
                     : prim == P_SEL8      ? kernel_of<P_SEL8>(nsets)
                     : prim == P_SEL16     ? kernel_of<P_SEL16>(nsets)
                     : prim == P_SEL16_SER ? kernel_of<P_SEL16_SER>(nsets)
                     : prim == P_KEEP8     ? kernel_of<P_KEEP8>(nsets)
                                           : kernel_of<P_KEEP16>(nsets);
    const double *ak = (const double *)dk.p, *af = (const double *)df.p;
    const uint8_t *am = (const uint8_t *)dm.p;
    int32_t *ap = (int32_t *)dp.p, *au = (int32_t *)du.p, *ai = (int32_t *)di.p, *ac = (int32_t *)dc.p;
    int aL = L, ags = gs;
    void *args[] = {&ak, &af, &am, &aL, &ags, &ap, &au, &ai, &ac};
    SEL_TRY(hipLaunchKernel(fn, dim3(nblocks), dim3(64), args, 0, nullptr));
    SEL_TRY(hipDeviceSynchronize());
    SEL_TRY(hipMemcpy(parent, dp.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    SEL_TRY(hipMemcpy(upper, du.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    SEL_TRY(hipMemcpy(ident, di.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    SEL_TRY(hipMemcpy(canary_ok, dc.p, (size_t)nblocks * sizeof(int32_t), hipMemcpyDeviceToHost));
#undef SEL_TRY
    return 0;
}

// The reference: mink on every lane group of `rows` rows of 64 lanes (groups of gs
// lanes, keys of the lanes gl < L; the others count as +inf padding and get -1).
int qpd_sel_reference(int L, int gs, int64_t rows, const double *keep, const double *flip, int32_t *parent,
                      int32_t *upper) {
    if (L < 1 || L > 16 || gs < L || gs > 64 || (gs & (gs - 1)) || rows < 0) return -1;
    std::vector<double> key(2 * L);
    std::vector<int> idx(2 * L);
    for (int64_t r = 0; r < rows; ++r)
        for (int g = 0; g < 64; g += gs) {
            const size_t at = (size_t)r * 64 + g;
            for (int i = 0; i < L; ++i) {
                key[i] = keep[at + i];
                key[L + i] = flip[at + i];
            }
            for (int i = 0; i < 2 * L; ++i) idx[i] = i;
            std::sort(idx.begin(), idx.end(), [&](int a, int b) { return key[a] < key[b]; });
            for (int i = 0; i < gs; ++i) {
                parent[at + i] = i < L ? (idx[i] < L ? idx[i] : idx[i] - L) : -1;
                upper[at + i] = i < L ? (idx[i] >= L ? 1 : 0) : -1;
            }
        }
    return 0;
}

// The emulator's predicate (tests/native/w16_replay_check.cpp): does the introsort's
// partitioning of a group's 2L keys, as far as it can reach the first L outputs
// (stl::partition_prefix), arrive at its depth limit?  fallback: [rows][4] flags, one
// per group of 16; partitions: [rows][4] partitions run before it stopped.
int qpd_sel_fallback(int L, int64_t rows, const double *keep, const double *flip, uint8_t *fallback,
                     int32_t *partitions) {
    namespace stl = qpd::stl;
    if (L < 9 || L > 16 || rows < 0) return -1;
    std::vector<double> key(2 * L);
    std::vector<int> idx(2 * L);
    for (int64_t r = 0; r < rows; ++r)
        for (int g = 0; g < 4; ++g) {
            const size_t at = (size_t)r * 64 + 16 * g;
            for (int i = 0; i < L; ++i) {
                key[i] = keep[at + i];
                key[L + i] = flip[at + i];
            }
            for (int i = 0; i < 2 * L; ++i) idx[i] = i;
            KeySeq s{idx.data(), key.data()};
            int f = 0, l = 2 * L, dl = stl::lg(2 * L) * 2, end = 2 * L, parts = 0;
            bool fell = false;
            while (l - f > stl::kThreshold) {
                if (dl == 0) {
                    fell = true;
                    break;
                }
                --dl;
                ++parts;
                stl::move_median_to_first(s, f, f + 1, f + (l - f) / 2, l - 1);
                const int cut = stl::unguarded_partition(s, f + 1, l, f);
                if (cut >= L && cut < end) end = cut;
                if (l - cut > stl::kThreshold) {
                    if (cut >= end) break;
                    f = cut;
                } else {
                    l = cut;
                }
            }
            fallback[r * 4 + g] = fell ? 1 : 0;
            if (partitions) partitions[r * 4 + g] = parts;
        }
    return 0;
}

// McIlroy's anti-quicksort adversary ("A Killer Adversary for Quicksort", 1999) run
// against this libstdc++'s std::sort on n elements: the n keys it settles on.
int qpd_sel_adversary(int n, double *out) {
    if (n < 2 || n > 32) return -1;
    std::vector<int> val(n, n - 1), idx(n);
    const int gas = n - 1;
    int nsolid = 0, candidate = 0;
    for (int i = 0; i < n; ++i) idx[i] = i;
    std::sort(idx.begin(), idx.end(), [&](int x, int y) {
        if (val[x] == gas && val[y] == gas) val[x == candidate ? x : y] = nsolid++;
        if (val[x] == gas) candidate = x;
        else if (val[y] == gas) candidate = y;
        return val[x] < val[y];
    });
    for (int i = 0; i < n; ++i) out[i] = (double)val[i];
    return 0;
}

}  // extern "C"
