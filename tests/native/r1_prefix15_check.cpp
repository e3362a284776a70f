// Host check of the R1 argsort of the fast kernel for up to 15 survivor layers
// (qpd_fast_special.hpp r1_prep with the layer bound 15: FastSCL-LUT, L = 9..16).  An R1
// node of n <= 32 elements sorts its |llr| with std::sort on an index array and a
// keys-only comparison (argsort, FastSCLLUTDecoder.cpp:7-17) and reads the first
// m = min(L - 1, n) outputs.  The kernel holds 16-bit entries rank << 5 | element
// (ranks < 16: one quanta row) and finds those m outputs in one of two ways,
// emulated here as one lane runs them:
//  * n <= 16 (std::sort is a stable insertion sort): m times the minimum of the
//    entries, the taken one set to 0xFFFF (the packed 16-bit min trees);
//  * 17 <= n <= 32: stl::partition_prefix on the entries (the introsort's
//    partitions as far as they can reach the first m outputs, heap-sort fallback
//    included), then m times the minimum of rank << 10 | position << 5 | element
//    over the positions [0, end).
// Both must give exactly the first m outputs of std::sort, for every m = 1..15,
// on tie-heavy, all-equal, sorted and reversed inputs, and on inputs that reach
// the introsort's depth limit (counted: the run fails if none did).
// usage: r1_prefix15_check [trials]; prints "mismatches=N heap_fallbacks=M".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "stl_sort.hpp"

struct EntrySeq {  // as LdsSeq16: entries rank << 5 | element, compared by their ranks only
    std::vector<int> &e;
    int get(int p) { return e[p]; }
    void set(int p, int v) { e[p] = v; }
    bool less(int a, int b) { return (a >> 5) < (b >> 5); }
};

// stl::partition_prefix's loop, only to see whether it takes the heap-sort fallback.
static bool reaches_heap_sort(std::vector<int> e, int m) {
    EntrySeq s{e};
    const int n = (int)e.size();
    int f = 0, l = n, dl = qpd::stl::lg(n) * 2, end = n;
    while (l - f > qpd::stl::kThreshold) {
        if (dl == 0) return true;
        --dl;
        qpd::stl::move_median_to_first(s, f, f + 1, f + (l - f) / 2, l - 1);
        const int cut = qpd::stl::unguarded_partition(s, f + 1, l, f);
        if (cut >= m && cut < end) end = cut;
        if (l - cut > qpd::stl::kThreshold) {
            if (cut >= end) break;
            f = cut;
        } else {
            l = cut;
        }
    }
    return false;
}

// n <= 16: the min-tree pick on (rank, element index)
static std::vector<int> pick_small(const std::vector<int> &rank, int m) {
    const int n = (int)rank.size();
    std::vector<uint16_t> ep(16, 0xFFFFu);
    for (int j = 0; j < n; ++j) ep[j] = (uint16_t)((rank[j] << 5) | j);
    std::vector<int> out;
    for (int q = 0; q < m && q < n; ++q) {
        uint16_t mn = 0xFFFFu;
        for (int j = 0; j < 16; ++j) mn = std::min(mn, ep[j]);
        out.push_back(mn & 31);
        for (int j = 0; j < 16; ++j)
            if (ep[j] == mn) ep[j] = 0xFFFFu;
    }
    return out;
}

// 17 <= n <= 32: partition_prefix, then the m smallest (rank, position) of [0, end)
static std::vector<int> pick_large(const std::vector<int> &rank, int m) {
    const int n = (int)rank.size();
    std::vector<int> e(n);
    for (int j = 0; j < n; ++j) e[j] = (rank[j] << 5) | j;
    EntrySeq s{e};
    const int end = qpd::stl::partition_prefix(s, 0, n, m);
    std::vector<uint16_t> ep(32, 0xFFFFu);
    for (int p = 0; p < end; ++p) ep[p] = (uint16_t)(((e[p] >> 5) << 10) | (p << 5) | (e[p] & 31));
    std::vector<int> out;
    for (int q = 0; q < m && q < n; ++q) {
        uint16_t mn = 0xFFFFu;
        for (int p = 0; p < 32; ++p) mn = std::min(mn, ep[p]);
        if (mn == 0xFFFFu) break;  // fewer than m entries before `end`: reported as a mismatch
        out.push_back(mn & 31);
        for (int p = 0; p < 32; ++p)
            if (ep[p] == mn) ep[p] = 0xFFFFu;
    }
    return out;
}

int main(int argc, char **argv) {
    const long trials = argc > 1 ? atol(argv[1]) : 40000;
    std::mt19937_64 rng(2024);
    long bad = 0, heaps = 0, small = 0, large = 0;
    // rank arrays (found by search) whose partitions each split off one or two elements, so that
    // the introsort spends its 2 lg(n) partitions above the threshold and falls back to heap sort
    const std::vector<std::vector<int>> fixed = {
        {10, 15, 1, 13, 5, 9, 1, 12, 8, 4, 9, 6, 7, 1, 5, 15, 7, 4, 11, 9, 8, 7, 9, 1, 9, 9, 9, 2, 1, 0, 0},
        {14, 0, 0, 1, 5, 12, 13, 6, 11, 8, 10, 7, 7, 8, 3, 15, 12, 5, 5, 5, 9, 10, 3, 8, 1, 3, 2, 1, 0, 14},
        {0, 14, 0, 13, 1, 9, 5, 15, 8, 5, 4, 4, 8, 6, 12, 3, 5, 8, 3, 4, 9, 4, 4, 2, 1, 12, 12, 0, 10, 13, 13},
    };
    for (long t = 0; t < trials + (long)fixed.size(); ++t) {
        std::vector<int> rank;
        if (t < (long)fixed.size()) {
            rank = fixed[t];
        } else {
            const int n = 1 + (int)(rng() % 32);
            const int mode = (int)(rng() % 6);
            const int distinct = 1 + (int)(rng() % 16);
            rank.resize(n);
            for (int &r : rank) r = (int)(rng() % distinct);
            if (mode == 1) std::fill(rank.begin(), rank.end(), (int)(rng() % 16));  // all equal
            if (mode == 2) std::sort(rank.begin(), rank.end());                     // sorted
            if (mode == 3) std::sort(rank.rbegin(), rank.rend());                   // reversed
            if (mode == 4)                                                          // organ pipe / sawtooth
                for (int i = 0; i < n; ++i) rank[i] = (t & 1) ? std::min(15, i < n / 2 ? i : n - i) : (i * 7) % 16;
            if (mode == 5 && n > 16) {  // a fixed array, a few entries changed
                rank = fixed[rng() % fixed.size()];
                for (int c = (int)(rng() % 3); c > 0; --c) rank[rng() % rank.size()] = (int)(rng() % 16);
            }
        }
        const int n = (int)rank.size();
        std::vector<int> ref(n);
        for (int i = 0; i < n; ++i) ref[i] = i;
        std::sort(ref.begin(), ref.end(), [&](int p, int q) { return rank[p] < rank[q]; });  // argsort
        (n <= qpd::stl::kThreshold ? small : large) += 1;
        bool heap = false;
        for (int m = 1; m <= 15; ++m) {
            const int k = std::min(m, n);
            if (n > qpd::stl::kThreshold) {
                std::vector<int> e(n);
                for (int j = 0; j < n; ++j) e[j] = (rank[j] << 5) | j;
                heap = heap || reaches_heap_sort(e, m);
            }
            const std::vector<int> got = n <= qpd::stl::kThreshold ? pick_small(rank, m) : pick_large(rank, m);
            if ((int)got.size() != k || !std::equal(got.begin(), got.end(), ref.begin())) {
                if (++bad < 5) {
                    printf("mismatch n=%d m=%d ranks:", n, m);
                    for (int r : rank) printf(" %d", r);
                    printf("\n");
                }
            }
        }
        heaps += heap;
    }
    printf("arrays=%ld (<=16: %ld, 17..32: %ld) mismatches=%ld heap_fallbacks=%ld\n", small + large, small, large, bad, heaps);
    if (heaps == 0) printf("no input reached the heap-sort fallback\n");
    return (bad || heaps == 0) ? 1 : 0;
}
