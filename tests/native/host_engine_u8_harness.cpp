// Test harness (CPU): the host engine's decode template on uint8 channel
// symbols (what qpd_decode_u8_host runs for small batches) beside its int32
// instantiation, built with g++ from csrc/qpd_host.hpp.
//
// Two builds of this file (tests/test_u8_input.py):
//  * a shared library: h8_decode decodes the same frames from an int32 and
//    from a uint8 copy with one plan and reports both results;
//  * with -DH8_MAIN a stand-alone program (own configurations, no Python) that
//    makes the same calls once -- the build the sanitizers run on.
#include <cstdio>
#include <cstring>
#include <vector>

#include "qpd_host.hpp"

// Decodes B frames twice: from sym32 (int32 [B][N]) into out32 and from sym8
// (uint8 [B][N]) into out8.  Returns -2 (no host plan) or the two engines'
// flags, int32's in bits 0-7 and uint8's in bits 8-15.
extern "C" int h8_decode(const qpd_config *c, const int32_t *sym32, const uint8_t *sym8, int64_t B, uint8_t *out32,
                         uint8_t *out8) {
    std::unique_ptr<qpd_host::Plan> p = qpd_host::make_plan(c);
    if (!p || p->dom != qpd::DOM_LUT) return -2;
    qpd_host::Engine<uint8_t> e32(*p), e8(*p);
    int f32 = 0, f8 = 0;
    for (int64_t b = 0; b < B; ++b) {
        f32 |= e32.decode(sym32 + b * p->N, out32 + b * p->out_k);
        f8 |= e8.decode(sym8 + b * p->N, out8 + b * p->out_k);
    }
    return (f32 & 255) | ((f8 & 255) << 8);
}

#ifdef H8_MAIN
namespace {

struct Rng {  // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    int below(int n) { return (int)(next() % (uint64_t)n); }
};

// Node labels as the drivers hand them to the Fast kinds: R0 0, R1 1, REP 2, SPC 3, -1 unlabelled
// (and below a labelled node); leaves 0 frozen / 1 information.
void label(std::vector<int32_t> &nt, const std::vector<int32_t> &frozen, int n, int depth, int node) {
    const int N = (int)frozen.size(), posi = (1 << depth) + node - 1, t = N >> depth;
    if (depth == n) {
        nt[posi] = frozen[node] == 0;
        return;
    }
    int s = 0;
    for (int i = 0; i < t; ++i) s += frozen[node * t + i] == 0;
    const bool last = frozen[node * t + t - 1] == 0, first = frozen[node * t] == 0;
    const int lab = s == 0 ? 0 : s == t ? 1 : (s == 1 && last) ? 2 : (s == t - 1 && !first) ? 3 : -1;
    if (lab >= 0) {
        nt[posi] = lab;
        return;
    }
    label(nt, frozen, n, depth + 1, 2 * node);
    label(nt, frozen, n, depth + 1, 2 * node + 1);
}

int run_case(int kind, int N, int v, int L, uint64_t seed) {
    Rng r{seed};
    int n = 0;
    while ((1 << n) < N) ++n;
    // a mask no Fast kind labels at the root: first position frozen, last two information, the rest random
    std::vector<int32_t> frozen(N);
    for (int i = 0; i < N; ++i) frozen[i] = r.below(2);
    frozen[0] = 1;
    frozen[1] = 0;
    frozen[N - 1] = frozen[N - 2] = 0;
    frozen[N / 2] = 1;
    int K = 0;
    for (int f : frozen) K += f == 0;
    std::vector<int32_t> nt(2 * N - 1, -1);
    label(nt, frozen, n, 0, 0);
    if (nt[0] >= 0) {
        std::fprintf(stderr, "harness mask labelled at the root\n");
        return 1;
    }
    // one table per node, tie-heavy quanta (three magnitudes)
    const size_t vv = (size_t)v * v;
    std::vector<uint8_t> lf((size_t)(N - 1) * vv), lg((size_t)(N - 1) * 2 * vv);
    for (auto &x : lf) x = (uint8_t)r.below(v);
    for (auto &x : lg) x = (uint8_t)r.below(v);
    std::vector<int32_t> base(N - 1);
    for (int p = 0; p < N - 1; ++p) base[p] = p;
    std::vector<double> vcl((size_t)n * N * v);
    for (auto &x : vcl) x = (r.below(2) ? 1.0 : -1.0) * (1 + r.below(3));
    qpd_config c;
    std::memset(&c, 0, sizeof(c));
    c.kind = kind;
    c.N = N, c.K = K, c.L = L, c.v = v;
    c.frozen_bits = frozen.data();
    c.node_type = nt.data();
    c.lut_f = lf.data(), c.lut_f_count = N - 1, c.f_base = base.data();
    c.lut_g = lg.data(), c.lut_g_count = N - 1, c.g_base = base.data();
    c.vcl = vcl.data(), c.vcl_rows = n;
    c.device = -1;
    const int B = 6;
    std::vector<int32_t> s32((size_t)B * N);
    std::vector<uint8_t> s8((size_t)B * N), o32((size_t)B * K, 7), o8((size_t)B * K, 9);
    for (size_t i = 0; i < s32.size(); ++i) s8[i] = (uint8_t)(s32[i] = r.below(v));
    s8[3] = (uint8_t)(s32[3] = v - 1);  // the largest symbol (255 at v = 256)
    int rc = h8_decode(&c, s32.data(), s8.data(), B, o32.data(), o8.data());
    if (rc != 0 || o32 != o8) {
        std::fprintf(stderr, "kind %d N %d v %d L %d: flags %d, outputs %s\n", kind, N, v, L, rc, o32 == o8 ? "equal" : "differ");
        return 1;
    }
    if (v < 256) {  // the symbol v: both readers report it
        s8[(size_t)2 * N + N / 2 + 1] = (uint8_t)(s32[(size_t)2 * N + N / 2 + 1] = v);
        rc = h8_decode(&c, s32.data(), s8.data(), B, o32.data(), o8.data());
        if (rc != (qpd::ERR_SYMBOL | (qpd::ERR_SYMBOL << 8))) {
            std::fprintf(stderr, "kind %d N %d v %d L %d: symbol v gave flags %d\n", kind, N, v, L, rc);
            return 1;
        }
    }
    return 0;
}

}  // namespace

int main() {
    int bad = 0, cases = 0;
    for (int kind : {QPD_SC_LUT, QPD_SCL_LUT, QPD_FASTSC_LUT, QPD_FASTSCL_LUT})
        for (int N : {8, 16, 128})
            for (int v : {2, 8, 16, 256})
                for (int L : {1, 4, 8}) {
                    bad += run_case(kind, N, v, L, 1000u * kind + 10u * N + v + L);
                    ++cases;
                }
    std::printf("host_engine_u8: %d cases, %d failed\n", cases, bad);
    return bad ? 1 : 0;
}
#endif
