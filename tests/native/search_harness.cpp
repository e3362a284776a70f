// Test harness (CPU): qpd_decode_search_host's host-engine branch without a device --
// the argument rules and the packed mask set (qpd_search.hpp: check) and the host
// engine's search run (host_run) exactly as qpd_capi.hip calls them, built with g++
// beside the tests like list_harness.cpp.  hs_decode_search returns the QPD_E_* code of
// a refusal, a positive qpd::ErrFlag for input the engine flags, else 0.
//
// With -DSEARCH_MAIN the file is also a stand-alone program for a sanitizer build
// (-fsanitize=address,undefined):
//     search_harness <case file>...
// Each case file (tests/test_search_host.py: write_case) holds a decoder configuration,
// frames, a mask set and the results the test has already compared with its numpy
// references; the program runs the search into heap blocks of exactly the outputs' sizes
// and compares.  Prints "search_harness: <n> cases, <m> failed"; exit status 1 when m > 0.
#include "qpd_search.hpp"

extern "C" int hs_decode_search(const qpd_config *c, const void *in, int32_t in_type, int64_t B, uint8_t *out,
                                const qpd_search_args *sa) {
    qpd_search::Req rq;
    std::string err;
    int fam = 0, dom = 0;
    const bool list = qpd_sched::family_of(c->kind, &fam, &dom) && (fam == QPD_SCL_LUT || fam == QPD_FASTSCL_LUT);
    const int rc = qpd_search::check(c->kind, list ? c->L : 1, c->K, c->A, c->crc_n, in_type, sa, out != nullptr, &rq, err);
    if (rc) return rc;
    std::unique_ptr<qpd_host::Plan> p = qpd_host::make_plan(c);
    if (!p) return QPD_E_UNSUPPORTED;
    if (p->dom == qpd::DOM_LUT) {
        qpd_host::Engine<uint8_t> e(*p);
        if (in_type == QPD_IN_U8) return qpd_search::host_run(&e, (const uint8_t *)in, B, p->N, p->L, p->out_k, out, rq);
        return qpd_search::host_run(&e, (const int32_t *)in, B, p->N, p->L, p->out_k, out, rq);
    }
    qpd_host::Engine<double> e(*p);
    return qpd_search::host_run(&e, (const double *)in, B, p->N, p->L, p->out_k, out, rq);
}

#ifdef SEARCH_MAIN
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

struct Reader {
    std::vector<char> buf;
    size_t at = 0;
    bool ok = true;
    template <class T>
    std::vector<T> arr(size_t n) {
        std::vector<T> v(n);
        if (at + n * sizeof(T) > buf.size()) {
            ok = false;
            return v;
        }
        if (n) std::memcpy(v.data(), buf.data() + at, n * sizeof(T));
        at += n * sizeof(T);
        return v;
    }
    int32_t i32() { return arr<int32_t>(1)[0]; }
};

// 1: the case failed (or could not be read)
int run_case(const char *path) {
    Reader r;
    FILE *f = std::fopen(path, "rb");
    if (!f) return 1;
    char tmp[65536];
    size_t n;
    while ((n = std::fread(tmp, 1, sizeof tmp, f)) > 0) r.buf.insert(r.buf.end(), tmp, tmp + n);
    std::fclose(f);
    qpd_config c{};
    c.kind = r.i32(), c.N = r.i32(), c.K = r.i32(), c.L = r.i32(), c.v = r.i32();
    c.A = r.i32(), c.crc_n = r.i32(), c.crc_loc_count = r.i32();
    c.lut_f_count = r.i32(), c.f_step = r.i32(), c.lut_g_count = r.i32(), c.g_step = r.i32(), c.vcl_rows = r.i32();
    const int has_nt = r.i32(), in_type = r.i32(), B = r.i32(), R = r.i32(), bits = r.i32(), want_rc = r.i32();
    if (!r.ok || c.N < 2 || c.N > 65536 || c.L < 1 || c.L > 32 || B < 0 || R < 0 || R > 4096 || bits < 0 || bits > 64) return 1;
    const size_t N = c.N, vv = (size_t)c.v * c.v;
    auto crc_loc = r.arr<int32_t>(c.crc_loc_count);
    auto frozen = r.arr<int32_t>(N);
    auto nt = r.arr<int32_t>(has_nt ? 2 * N - 1 : 0);
    auto lut_f = r.arr<uint8_t>((size_t)c.lut_f_count * vv);
    auto f_base = r.arr<int32_t>(c.lut_f_count ? N - 1 : 0);
    auto lut_g = r.arr<uint8_t>((size_t)c.lut_g_count * 2 * vv);
    auto g_base = r.arr<int32_t>(c.lut_g_count ? N - 1 : 0);
    auto vcl = r.arr<double>((size_t)c.vcl_rows * N * c.v);
    const size_t esz = in_type == QPD_IN_F64 ? 8 : in_type == QPD_IN_U8 ? 1 : 4;
    auto x = r.arr<uint8_t>((size_t)B * N * esz);
    auto masks = r.arr<uint8_t>((size_t)R * bits);
    const size_t nl = (size_t)B * c.L, no = R ? (size_t)B : 0;
    auto w_syn = r.arr<uint32_t>(nl);
    auto w_cm = r.arr<double>(nl);
    auto w_hit = r.arr<int32_t>(no);
    auto w_rank = r.arr<int32_t>(no);
    auto w_met = r.arr<double>(no);
    auto w_out = r.arr<uint8_t>(no * (size_t)c.A);
    if (!r.ok || r.at != r.buf.size()) return 1;
    c.crc_loc = crc_loc.data();
    c.frozen_bits = frozen.data();
    c.node_type = has_nt ? nt.data() : nullptr;
    c.lut_f = lut_f.data(), c.f_base = f_base.data(), c.lut_g = lut_g.data(), c.g_base = g_base.data(), c.vcl = vcl.data();
    // the outputs in heap blocks of exactly their sizes (vectors), so that a write past one is caught
    std::vector<uint32_t> syn(nl);
    std::vector<double> cm(nl), met(no);
    std::vector<int32_t> hit(no), rank(no);
    std::vector<uint8_t> out(no * (size_t)c.A);
    qpd_search_args sa{};
    sa.crc_masks = masks.empty() ? nullptr : masks.data();
    sa.n_masks = R, sa.crc_mask_bits = bits;
    sa.cand_syndrome = syn.data(), sa.cand_metric = cm.data();
    if (R) sa.hit_mask = hit.data(), sa.hit_rank = rank.data(), sa.metric = met.data();
    const int rc = hs_decode_search(&c, x.data(), in_type, B, R ? out.data() : nullptr, &sa);
    if (rc != want_rc) return 1;
    if (rc) return 0;
    // the metrics as the same doubles (bit patterns; vectors compare by ==, and no metric is a NaN)
    return !(syn == w_syn && cm == w_cm && hit == w_hit && rank == w_rank && met == w_met && out == w_out);
}

}  // namespace

int main(int argc, char **argv) {
    int failed = 0;
    for (int i = 1; i < argc; ++i) {
        const int f = run_case(argv[i]);
        if (f) std::printf("FAILED %s\n", argv[i]);
        failed += f;
    }
    std::printf("search_harness: %d cases, %d failed\n", argc - 1, failed);
    return failed ? 1 : 0;
}
#endif
