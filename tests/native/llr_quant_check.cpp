// llr_quant_check -- the shared channel quantizer (csrc/qpd_llr_quant.hpp, the text
// the front kernel and the host entry point call) against a literal restatement of
// the driver's loop (mainQuantizedDecoder_LLRDomain.py:167-176).  Host code, plain
// g++; may be built with -fsanitize=address,undefined.
//
//   llr_quant_check <in> <out>
// <in>:  text -- q n_edges, the edges (%la), the lut, then n and n LLRs as raw
//        uint64 bit patterns (hex), each also tried as the widened float32 nearest
//        to it where that float32's double equals an edge;
// <out>: one symbol per LLR (-1: NaN), as the shared function computed it.
// Exit status 1 and a message on the first disagreement with the restatement.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "qpd_llr_quant.hpp"

// bisect.bisect_left(a[0:n], x): CPython's loop.
static int bisect_left(const double *a, int n, double x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (a[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// The driver's loop body for one LLR (not a NaN).
static int driver(double x, const std::vector<double> &edges, const std::vector<int32_t> &lut, int q) {
    const int M = (int)edges.size() - 1;
    if (x <= edges[0]) return 0;
    if (x >= edges[M]) return q - 1;
    return lut[bisect_left(edges.data(), M, x) - 1];
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *fi = std::fopen(argv[1], "r");
    if (!fi) return 2;
    int q = 0, ne = 0;
    if (std::fscanf(fi, "%d %d", &q, &ne) != 2 || ne < 2 || ne > qpd::kLlrMaxEdges) return 2;
    std::vector<double> edges(ne);
    std::vector<int32_t> lut(ne - 1);
    for (double &e : edges)
        if (std::fscanf(fi, "%la", &e) != 1) return 2;
    for (int32_t &l : lut)
        if (std::fscanf(fi, "%" SCNd32, &l) != 1) return 2;
    long n = 0;
    if (std::fscanf(fi, "%ld", &n) != 1 || n < 0) return 2;
    std::vector<double> x(n);
    for (double &v : x) {
        uint64_t b;
        if (std::fscanf(fi, "%" SCNx64, &b) != 1) return 2;
        std::memcpy(&v, &b, sizeof v);
    }
    std::fclose(fi);

    const qpd::LlrQuant Q = qpd::llr_quant_params(edges.data(), ne, q);
    std::vector<double> E(ne + 1);  // exactly M + 2 entries: a read past the guards is the sanitizer's
    qpd::llr_guard_edges(edges.data(), ne, E.data());
    std::vector<uint8_t> lut8(lut.begin(), lut.end());  // the kernel's byte lut
    FILE *fo = std::fopen(argv[2], "w");
    if (!fo) return 2;
    long checked = 0;
    auto check = [&](double v, const char *what) -> int {
        const int s = qpd::quantize_llr(v, Q, E.data(), lut.data());
        const int s8 = qpd::quantize_llr(v, Q, E.data(), lut8.data());
        const int want = v != v ? -1 : driver(v, edges, lut, q);
        ++checked;
        if (s != want || s8 != want) {
            std::fprintf(stderr, "%s %a: shared %d / %d, driver %d\n", what, v, s, s8, want);
            return -2;
        }
        return s;
    };
    for (double v : x) {
        const int s = check(v, "llr");
        if (s == -2) return 1;
        std::fprintf(fo, "%d\n", s);
        // float32 input: the value the kernel widens.  Only exact widenings are new cases
        const float f = (float)v;
        if (check((double)f, "float32") == -2) return 1;
    }
    // float32 values whose widened double equals an edge, and their float32 neighbours
    for (double e : edges) {
        const float f = (float)e;
        if ((double)f != e) continue;
        const float nb[3] = {f, std::nextafterf(f, -INFINITY), std::nextafterf(f, INFINITY)};
        for (float g : nb)
            if (check((double)g, "float32 at an edge") == -2) return 1;
    }
    std::fclose(fo);
    std::printf("%ld\n", checked);
    return 0;
}
