// Test harness (CPU): qpd_dmetric_host's host-engine branch without a device -- the
// argument rules (qpd_dmetric.hpp: check) and the host engine's metric run
// (host_run) exactly as qpd_capi.hip calls them.  A program of its own, built with
// g++ beside the tests from the library's sources:
//     dmetric_harness CASE RESULT
// CASE (little endian): int32 kind, N, K, B, want_bits, null_metric; int32 frozen[N];
// int32 node_type[2N-1]; double llr[B][N].  RESULT: int32 rc (the QPD_E_* code of a
// refusal, a positive qpd::ErrFlag for input the engine flags, else 0), then, for
// rc == 0, double metric[B] and, with want_bits, uint8 bits[B][K].  A refusal's
// message goes to stdout.
#include <cstdio>
#include <vector>

#include "qpd_dmetric.hpp"

template <class T>
static bool get(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<int32_t> h, frozen, node_type;
    std::vector<double> llr;
    if (!get(in, h, 6) || h[1] < 2 || h[1] > 65536 || h[3] < 0) return 2;
    const int kind = h[0], N = h[1], K = h[2];
    const int64_t B = h[3];
    const bool want_bits = h[4] != 0, null_metric = h[5] != 0;
    if (!get(in, frozen, (size_t)N) || !get(in, node_type, (size_t)2 * N - 1) || !get(in, llr, (size_t)B * N)) return 2;
    fclose(in);

    std::vector<double> metric((size_t)B, -1.0);
    std::vector<uint8_t> bits(want_bits ? (size_t)B * K : 0, 7);
    std::string err;
    int32_t rc = qpd_dm::check(kind, null_metric ? nullptr : metric.data(), err);
    if (rc) {
        printf("%s\n", err.c_str());
    } else {
        qpd_config c{};
        c.kind = kind;
        c.N = N;
        c.K = K;
        c.L = 1;
        c.frozen_bits = frozen.data();
        c.node_type = node_type.data();
        std::unique_ptr<qpd_host::Plan> p = qpd_host::make_plan(&c);
        if (!p || p->out_k != K) return 2;
        qpd_host::Engine<double> e(*p);
        rc = qpd_dm::host_run(&e, llr.data(), B, N, p->out_k, metric.data(), want_bits ? bits.data() : nullptr);
    }
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    fwrite(&rc, sizeof(rc), 1, out);
    if (rc == 0) {
        fwrite(metric.data(), sizeof(double), metric.size(), out);
        fwrite(bits.data(), 1, bits.size(), out);
    }
    fclose(out);
    return 0;
}
