// Scalar emulation of the W16 survivor selection (qpd_fast_select.hpp select_survivors16:
// dense key ranks, the group-parallel replay of stl::partition_prefix by scan-stop
// masks and all of a partition's swaps at once (stop ranks and slots), and the
// final (rank, position) selection), step for step as one lane group runs it,
// checked against std::sort on the 2L candidate indices (mink,
// SCLLUTDecoder.cpp:8-21) -- the first L outputs must be identical.
//
// A group whose replay arrives at the introsort's depth limit leaves the parallel
// replay: its first lane runs stl::sort_small_prefix (stl_sort.hpp, heap-sort fallback
// included) on the original keys.  Such a case is checked here in the same way, that
// call against std::sort, and counted; the emulation's "depth limit reached" must
// also agree with stl::partition_prefix's own loop on the keys.
//
// The depth limit is 2 lg(2L) partitions with more than 16 elements left, and every
// partition takes at least one element off the range: 2L - 2 lg(2L) >= 17 needs
// 2L >= 26, so L = 9..12 cannot reach it on any input; L = 13..16 can.
//
// Inputs:
//  * random: path-metric-like keys (keeps roughly ascending, flips = keep + penalty)
//    drawn from few distinct values (ties at almost every selection), all-equal and
//    +inf keys.  None of these reaches the depth limit (fallbacks stay 0 over
//    millions of them), so the limit is reached by construction:
//  * the deep-partition rank arrays of r1_prefix15_check.cpp whose length is an even
//    2L (one: 30 entries, L = 15), used as 2L keys;
//  * McIlroy's anti-quicksort adversary ("A Killer Adversary for Quicksort", 1999) run
//    against std::sort itself for every 2L -- it makes the partitions lopsided but, with
//    median-of-3 on 18..32 elements, does not reach the limit on its own;
//  * every single-entry mutation of both;
//  * a search for depth-limit witnesses at each L = 13..16, bounded by a fixed number
//    of probes (not by time): hill climbing on the sum of the partitioned range sizes.
// usage: w16_replay_check [trials] [witness-file] [probes per L]; prints per L the
// deepest partition count seen and the fallbacks, then "trials=N mismatches=N
// fallbacks=M"; with a file name, writes the witnesses found (a few per L) as JSON
// arrays of 2L keys.  Fails on a mismatch and when nothing reached the depth limit.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "stl_sort.hpp"

namespace stl = qpd::stl;

struct KeySeq {  // mink's index array: candidate indices compared by their keys
    std::vector<int> &idx;
    const std::vector<double> &key;
    int get(int p) { return idx[p]; }
    void set(int p, int e) { idx[p] = e; }
    bool less(int a, int b) { return key[a] < key[b]; }
};

// Returns false when the replay needs its serial fallback (the depth limit);
// `parts`: the partitions it ran.
static bool emulate(const std::vector<double> &key, int L, std::vector<int> &out, int &parts) {
    const int n2 = 2 * L;
    std::vector<uint32_t> lt(n2), ent(n2);
    for (int i = 0; i < n2; ++i) {
        int c = 0;
        for (int j = 0; j < n2; ++j) c += key[j] < key[i];
        lt[i] = (uint32_t)c;
        ent[i] = (lt[i] << 5) | (uint32_t)i;  // position i holds candidate i
    }
    int f = 0, l = n2, dl = 2 * stl::lg(n2), end = n2;
    bool live = true;
    parts = 0;
    while (live) {
        if (dl == 0) return false;
        --dl;
        ++parts;
        const int mid = f + (l - f) / 2;
        const uint32_t ea = ent[f + 1], eb = ent[mid], ec = ent[l - 1], ef = ent[f];
        const uint32_t ra = ea >> 5, rb = eb >> 5, rc = ec >> 5;
        int pick;
        if (ra < rb) pick = rb < rc ? mid : ra < rc ? l - 1 : f + 1;
        else pick = ra < rc ? f + 1 : rb < rc ? l - 1 : mid;
        const uint32_t em = pick == mid ? eb : pick == f + 1 ? ea : ec;
        ent[f] = em;
        ent[pick] = ef;
        const uint32_t pv = em >> 5;
        const uint32_t in = ((l < 32 ? (1u << l) : 0u) - 1u) & ~((2u << f) - 1u);
        uint32_t GE = 0, LE = 0;
        for (int p = 0; p < n2; ++p) {
            GE |= (uint32_t)((ent[p] >> 5) >= pv) << p;
            LE |= (uint32_t)((ent[p] >> 5) <= pv) << p;
        }
        GE &= in;
        LE &= in;
        // all swaps at once, as the kernel: ranks, byte slots, partners
        int slotA[32], slotB[32];
        for (int p = 0; p < n2; ++p) {
            if ((GE >> p) & 1u) slotA[__builtin_popcount(GE & ((1u << p) - 1u))] = p;
            if ((LE >> p) & 1u) slotB[__builtin_popcount(LE & ~((p < 31 ? (2u << p) : 0u) - 1u))] = p;
        }
        const int nA = __builtin_popcount(GE), nB = __builtin_popcount(LE);
        std::vector<uint32_t> nxt(ent);
        int S = 0;
        for (int p = 0; p < n2; ++p) {
            const int kA = __builtin_popcount(GE & ((1u << p) - 1u));
            const int kB = __builtin_popcount(LE & ~((p < 31 ? (2u << p) : 0u) - 1u));
            const int bk = ((GE >> p) & 1u) && kA < nB ? slotB[kA] : -1;
            const int ak = ((LE >> p) & 1u) && kB < nA ? slotA[kB] : 64;
            if (p < bk) {
                nxt[p] = ent[bk];
                ++S;
            } else if (ak < p) {
                nxt[p] = ent[ak];
            }
        }
        ent = nxt;
        const int cut_a = S < nA ? slotA[S] : n2, cut_b = S >= 1 ? slotB[S - 1] : n2;
        const int cut = cut_a < cut_b ? cut_a : cut_b;
        if (cut >= L && cut < end) end = cut;
        if (l - cut > 16) {
            if (cut >= end) live = false;
            else f = cut;
        } else {
            l = cut;
        }
        live = live && l - f > 16;
    }
    std::vector<uint32_t> comp(n2);
    for (int p = 0; p < n2; ++p) comp[p] = p < end ? ((ent[p] & 0xFFE0u) | (uint32_t)p) : 0xFFFFu;
    out.assign(L, -1);
    for (int p = 0; p < n2; ++p) {
        int r = 0;
        for (int q = 0; q < n2; ++q) r += comp[q] < comp[p];
        if (r < L) out[r] = (int)(ent[p] & 31u);
    }
    return true;
}

// stl::partition_prefix's own loop on the keys: does it take the heap-sort fallback;
// `weight`: the sum of the range sizes it partitioned (the search's objective).
static bool reaches_limit(const std::vector<double> &key, int L, int &weight) {
    const int n2 = 2 * L;
    std::vector<int> idx(n2);
    for (int i = 0; i < n2; ++i) idx[i] = i;
    KeySeq s{idx, key};
    int f = 0, l = n2, dl = stl::lg(n2) * 2, end = n2;
    weight = 0;
    while (l - f > stl::kThreshold) {
        if (dl == 0) return true;
        --dl;
        weight += l - f;
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
    return false;
}

struct Tally {
    long total = 0, mism = 0, fall = 0;
    long fall_L[17] = {}, cases_L[17] = {};
    int deepest_L[17] = {};
    std::map<int, std::set<std::vector<double>>> witnesses;
};

static void report(const char *what, const std::vector<double> &key, int L, Tally &t) {
    if (t.mism++ < 5) {
        printf("mismatch (%s) L=%d keys:", what, L);
        for (double k : key) printf(" %g", k);
        printf("\n");
    }
}

// One group's 2L keys through everything the kernel can run on them.
static void check(const std::vector<double> &key, int L, Tally &t) {
    const int n2 = 2 * L;
    std::vector<int> ref(n2);
    for (int i = 0; i < n2; ++i) ref[i] = i;
    std::sort(ref.begin(), ref.end(), [&](int p, int q) { return key[p] < key[q]; });  // mink
    ++t.total;
    ++t.cases_L[L];
    // the serial replay (the kernel's first lane on a fallback group): checked on every input
    std::vector<int> idx(n2);
    for (int i = 0; i < n2; ++i) idx[i] = i;
    KeySeq seq{idx, key};
    stl::sort_small_prefix(seq, 0, n2, L);
    const bool serial_ok = std::equal(idx.begin(), idx.begin() + L, ref.begin());
    std::vector<int> got;
    int parts = 0, weight = 0;
    const bool parallel = emulate(key, L, got, parts);
    const bool limit = reaches_limit(key, L, weight);
    t.deepest_L[L] = std::max(t.deepest_L[L], parts);
    if (parallel == limit) return report("depth-limit predicate", key, L, t);
    if (!parallel) {
        ++t.fall;
        ++t.fall_L[L];
        if (t.witnesses[L].size() < 6) t.witnesses[L].insert(key);
        if (!serial_ok) report("serial fallback", key, L, t);
        return;
    }
    if (!serial_ok) return report("serial replay", key, L, t);
    if (!std::equal(got.begin(), got.end(), ref.begin())) report("parallel replay", key, L, t);
}

// McIlroy's adversary against std::sort on n elements: the keys it settles on.
namespace adversary {
static std::vector<int> val;
static int nsolid, candidate, gas;
static bool less(int x, int y) {
    if (val[x] == gas && val[y] == gas) val[x == candidate ? x : y] = nsolid++;
    if (val[x] == gas) candidate = x;
    else if (val[y] == gas) candidate = y;
    return val[x] < val[y];
}
static std::vector<double> keys(int n) {
    gas = n - 1;
    nsolid = candidate = 0;
    val.assign(n, gas);
    std::vector<int> idx(n);
    for (int i = 0; i < n; ++i) idx[i] = i;
    std::sort(idx.begin(), idx.end(), less);
    return std::vector<double>(val.begin(), val.end());
}
}  // namespace adversary

static void mutations(const std::vector<double> &base, int nvals, Tally &t) {
    const int L = (int)base.size() / 2;
    check(base, L, t);
    for (size_t p = 0; p < base.size(); ++p)
        for (int v = 0; v < nvals; ++v) {
            std::vector<double> k(base);
            k[p] = (double)v;
            check(k, L, t);
        }
}

// Hill climbing towards the depth limit at one L, `probes` evaluations in all.
static void search(int L, long probes, const std::vector<std::vector<double>> &seeds, Tally &t) {
    const int n2 = 2 * L;
    std::mt19937_64 rng(977 * L);
    std::vector<double> cur;
    int cur_w = -1;
    long stale = 0, restarts = 0;
    for (long it = 0; it < probes; ++it) {
        if (cur_w < 0 || stale > 4000) {  // (re)start: a seed resized to 2L, or random ranks
            if (restarts < (long)seeds.size()) {
                cur = seeds[restarts];
                while ((int)cur.size() > n2) cur.erase(cur.begin() + (long)(rng() % cur.size()));
                while ((int)cur.size() < n2) cur.insert(cur.begin() + (long)(rng() % (cur.size() + 1)), (double)(rng() % 16));
            } else {
                cur.resize(n2);
                const int nv = 2 + (int)(rng() % 15);
                for (double &k : cur) k = (double)(rng() % nv);
            }
            ++restarts;
            stale = 0;
            reaches_limit(cur, L, cur_w);
        }
        std::vector<double> cand(cur);
        for (int c = 1 + (int)(rng() % 2); c > 0; --c) {
            const size_t p = rng() % n2;
            cand[p] = rng() % 3 ? (double)(rng() % 16) : cand[rng() % n2];
        }
        int w = 0;
        if (reaches_limit(cand, L, w)) {
            check(cand, L, t);  // a witness: through the whole check, and recorded
            cur_w = -1;
            continue;
        }
        if (w >= cur_w) {
            stale = w > cur_w ? 0 : stale + 1;
            cur = cand;
            cur_w = w;
        } else {
            ++stale;
        }
    }
}

int main(int argc, char **argv) {
    const int trials = argc > 1 ? atoi(argv[1]) : 20000;
    const char *dump = argc > 2 && argv[2][0] ? argv[2] : nullptr;
    const long probes = argc > 3 ? atol(argv[3]) : 150000;  // per L: the search's fixed budget
    std::mt19937_64 rng(12345);
    Tally t;
    const double inf = INFINITY;
    for (int n = 0; n < trials; ++n) {
        const int L = 9 + (int)(rng() % 8);
        const int n2 = 2 * L;
        std::vector<double> key(n2);
        const int mode = (int)(rng() % 6);
        const int nv = 1 + (int)(rng() % 5);
        for (int j = 0; j < L; ++j) {
            double k;
            switch (mode) {
                case 0: k = (double)(rng() % nv); break;                              // few values, any order
                case 1: k = (double)(j / (1 + (int)(rng() % 3))); break;              // ascending keeps with runs
                case 2: k = j < (int)(rng() % L) ? (double)(rng() % 3) : inf; break;  // dead paths
                case 3: k = 7.0; break;                                               // all equal
                case 4: k = (double)((j * 7919) % 11 < 4 ? j % 3 : 10 + j); break;    // mixed
                default: k = std::ldexp((double)(rng() % 8), -(int)(rng() % 3)); break;
            }
            key[j] = k;
        }
        for (int j = 0; j < L; ++j) {
            const double pen = (mode == 3 || rng() % 4 == 0) ? 0.0 : (double)(1 + rng() % nv);
            key[L + j] = key[j] + pen;
        }
        check(key, L, t);
    }
    const long random_falls = t.fall;
    // the deep-partition rank arrays of r1_prefix15_check.cpp (found by search there)
    const std::vector<std::vector<double>> fixed = {
        {10, 15, 1, 13, 5, 9, 1, 12, 8, 4, 9, 6, 7, 1, 5, 15, 7, 4, 11, 9, 8, 7, 9, 1, 9, 9, 9, 2, 1, 0, 0},
        {14, 0, 0, 1, 5, 12, 13, 6, 11, 8, 10, 7, 7, 8, 3, 15, 12, 5, 5, 5, 9, 10, 3, 8, 1, 3, 2, 1, 0, 14},
        {0, 14, 0, 13, 1, 9, 5, 15, 8, 5, 4, 4, 8, 6, 12, 3, 5, 8, 3, 4, 9, 4, 4, 2, 1, 12, 12, 0, 10, 13, 13},
    };
    for (const auto &a : fixed)
        if (a.size() % 2 == 0 && a.size() >= 18 && a.size() <= 32) mutations(a, 16, t);
    for (int L = 9; L <= 16; ++L) mutations(adversary::keys(2 * L), 2 * L, t);
    for (int L = 13; L <= 16; ++L) search(L, probes, fixed, t);
    for (int L = 9; L <= 16; ++L)
        printf("L=%d cases=%ld deepest_partitions=%d (limit %d) fallbacks=%ld\n", L, t.cases_L[L], t.deepest_L[L],
               2 * stl::lg(2 * L), t.fall_L[L]);
    printf("random_fallbacks=%ld\n", random_falls);
    printf("trials=%ld mismatches=%ld fallbacks=%ld\n", t.total, t.mism, t.fall);
    if (dump) {
        FILE *fh = fopen(dump, "w");
        if (!fh) return 2;
        fprintf(fh, "{\n");
        bool first = true;
        for (const auto &kv : t.witnesses) {
            fprintf(fh, "%s \"%d\": [\n", first ? "" : ",\n", kv.first);
            first = false;
            size_t i = 0;
            for (const auto &k : kv.second) {
                fprintf(fh, "  [");
                for (size_t j = 0; j < k.size(); ++j) fprintf(fh, "%s%g", j ? ", " : "", k[j]);
                fprintf(fh, "]%s\n", ++i < kv.second.size() ? "," : "");
            }
            fprintf(fh, " ]");
        }
        fprintf(fh, "\n}\n");
        fclose(fh);
    }
    return (t.mism != 0 || t.fall == 0) ? 1 : 0;
}
