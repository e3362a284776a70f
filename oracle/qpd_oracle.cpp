// =============================================================================
// qpd_oracle.cpp -- CPU restatement of the reference polar decoders.
//
// TEST INFRASTRUCTURE ONLY.  This file is the parity checker for the HIP
// product path and the `cpu_baseline` leg of bench.py.  Nothing in
// quantized_decoder_polar_codes_amd/ links, loads or calls it.  It restates,
// from scratch and in its own structure (explicit recursion instead of the
// reference's node_state machine), the algorithms of
//
//   SC   (float)    /root/reference/PolarDecoder/PolarDecoder/_cpp/src/SCDecoder.cpp:14-89
//   SC-LUT          .../src/SCLUTDecoder.cpp:21-124
//   SCL-LUT         .../src/SCLLUTDecoder.cpp:47-253   (mink :8-21, argmin :25-29)
//   FastSC-LUT      .../src/FastSCLUT.cpp:27-206
//   FastSCL-LUT     .../src/FastSCLLUTDecoder.cpp:57-408 (argsort :7-17)
//   CA-SCL-LUT      .../src/CASCLLUTDecoder.cpp:47-303   (CRC epilogue :263-302)
//   CA-FastSCL-LUT  .../src/CAFastSCLLUTDecoder.cpp:57-454 (CRC epilogue :332-453)
//   CRC::encoding   .../src/utils.cpp:77-92
//   SCL (float)     .../src/SCLDecoder.cpp:38-176
//   CA-SCL (float)  .../src/CASCLDecoder.cpp:56-249
//   FastSC (float)  .../src/FastSCDecoder.cpp:21-174
//   FastSCL (float) .../src/FastSCLDecoder.cpp:49-423
//   SC/SCL uniform  .../src/SC{,L}UniformQuantizedDecoder.cpp (Q utils.cpp:8-10)
//   SC/SCL Lloyd    .../src/SC{,L}{l,L}loydQuantizedDecoder.cpp (bisect utils.cpp:12-24)
//   partial sums    .../src/utils.cpp:62-67 (u), min-sum f/g utils.cpp:26-36
//
// One template per decoder family (SCDec / SCLDec) over a symbol domain
// (LutDom: int symbols + tables; FloatDom: fp64 LLRs, min-sum, optional
// uniform / Lloyd re-quantization), since the reference's 15 classes differ
// only in those two respects.  It keeps the reference's per-fork deep copies of the whole list state, so
// that its speed is representative of the reference CPU decoder (SURVEY.md
// §8(d)), and it calls libstdc++ std::sort with the same comparator as the
// reference so that tie order is identical (hazard H1).  Parity is pinned by
// tests/test_oracle_vs_reference.py against the reference compiled from its
// own sources (oracle/build_ref.sh -> oracle/_ref/).
//
// Table layout shared with the product C-ABI (include/qpd.h):
//   f table t : lut_f[t*v*v + a*v + b]                     (a = first half)
//   g table t : lut_g[(t*2 + u)*v*v + a*v + b]
//   node p (node_posi = 2^depth + node - 1), element j uses table
//        f_base[p] + j*f_step   (f_step 0 = one table per node, 1 = per element)
//   vcl       : vcl[((row*N) + pos)*v + sym], rows = vcl_rows
// =============================================================================
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

namespace {

struct Code {
    int N, K, L, v, n;
    const int32_t *frozen;
    const int32_t *node_type;  // may be null (no special nodes)
    const uint8_t *lut_f;
    const int32_t *f_base;
    int f_step;
    const uint8_t *lut_g;
    const int32_t *g_base;
    int g_step;
    const double *vcl;
    int vcl_rows;

    int F(int posi, int j, int a, int b) const {
        size_t t = (size_t)f_base[posi] + (size_t)j * f_step;
        return lut_f[t * v * v + (size_t)a * v + b];
    }
    int G(int posi, int j, int u, int a, int b) const {
        size_t t = (size_t)g_base[posi] + (size_t)j * g_step;
        return lut_g[(t * 2 + u) * v * v + (size_t)a * v + b];
    }
    double Q(int row, int pos, int sym) const {
        return vcl[((size_t)row * N + pos) * v + sym];
    }
    int type(int posi) const { return node_type ? node_type[posi] : -1; }
};

const double kInf = std::numeric_limits<double>::infinity();

int ilog2(int N) {
    int n = 0;
    while ((1 << n) < N) ++n;
    return n;
}

// Partial-sum combine, utils.cpp:62-67: out = [l ^ r, r].
void combine(uint8_t *out, const uint8_t *l, const uint8_t *r, int half) {
    for (int j = 0; j < half; ++j) out[j] = l[j] ^ r[j];
    std::memcpy(out + half, r, half);
}

// Polar re-encoding of the root partial sums, FastSCLUT.cpp:186-198.
void reencode(std::vector<uint8_t> &x, int N) {
    for (int m = 1; m < N; m *= 2)
        for (int i = 0; i < N; i += 2 * m)
            for (int j = 0; j < m; ++j) x[i + j] ^= x[i + m + j];
}

void emit_info(const Code &c, const uint8_t *bits, uint8_t *out) {
    int t = 0;
    for (int i = 0; i < c.N; ++i)
        if (c.frozen[i] == 0) out[t++] = bits[i];
}

// std::sort of an index vector by key -- the reference's mink/argsort
// (SCLLUTDecoder.cpp:8-21, FastSCLLUTDecoder.cpp:7-34).  Same libstdc++ call,
// same comparator, hence the same order among ties.
std::vector<int> sort_index(const std::vector<double> &key) {
    std::vector<int> idx(key.size());
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = (int)i;
    std::sort(idx.begin(), idx.end(), [&key](int p, int q) { return key[p] < key[q]; });
    return idx;
}

// CRC::encoding, utils.cpp:77-92: long division of info || 0^crc_n by the
// coefficient vector p (p[loc] = 1, utils.cpp:69-75); returns the crc_n bits
// that follow the info bits after the division.
std::vector<uint8_t> crc_encoding(const std::vector<uint8_t> &info, int crc_n, const std::vector<int> &p) {
    const int A = (int)info.size();
    std::vector<uint8_t> u(A + crc_n, 0);
    std::memcpy(u.data(), info.data(), A);
    for (int i = 0; i < A; ++i)
        if (u[i] == 1)
            for (int j = 0; j <= crc_n; ++j) u[j + i] = (uint8_t)((u[j + i] + p[j]) % 2);
    return std::vector<uint8_t>(u.begin() + A, u.end());
}

// CRC-aided list output (CASCLLUTDecoder.cpp:263-302): walk the paths in
// argsort(PML) order (L <= 8: libstdc++ insertion sort, stable, H1); the
// first whose decoded info bits [0, A) reproduce bits [A, K) under the CRC
// wins, else the first in that order.
struct CaSpec {
    int A = 0, crc_n = 0;
    int nchk = 0;  // bits compared after the A info bits: K - A (LUT kinds,
                   // CASCLLUTDecoder.cpp:279) or crc_n (CASCLDecoder.cpp:223)
    std::vector<int> p;  // crc_n + 1 coefficients
    std::vector<uint8_t> mask;  // 0 / 1, XORed onto check-code bits [crc_n - size, crc_n) (CASCLWithRNTI.cpp:222-224)
};

// What a list decode knows at its end beside the output bits.
struct Status {
    std::vector<double> pml;  // every path's final metric, in path-index order
    int winner = 0;           // index of the output path
    bool passed = false;      // CRC-aided: the output path's compare succeeded
};

int first_argmin(const std::vector<double> &x) {
    return (int)std::distance(x.begin(), std::min_element(x.begin(), x.end()));
}

// ---------------------------------------------------------------------------
// Symbol domains.  The reference's decoders differ only in what a tree node
// holds and how f/g and a node's LLR are formed:
//   LutDom   -- int symbols, f/g by per-node tables, LLR = vcl[row][pos][sym]
//               (SCLUTDecoder.cpp:83-97, hazard H3: row depth-1)
//   FloatDom -- fp64 LLRs, min-sum f/g (utils.cpp:26-36), optionally
//               re-quantized after every f/g: uniform Q (utils.cpp:8-10,
//               q_f/q_g :38-48, SCUniformQuantizedDecoder.cpp:55-57,71-73) or
//               Lloyd bisect (utils.cpp:12-24, non_uniform_q_f/g :50-60,
//               SCLloydQuantizedDecoder.cpp:57-59,73-75); LLR = the value.
// ---------------------------------------------------------------------------
int sgn(double x) { return x < 0 ? -1 : (x > 0); }  // utils.h:13

struct LutDom {
    using T = int;
    const Code &c;
    T f(int posi, int j, T a, T b) const { return c.F(posi, j, a, b); }
    T g(int posi, int j, int u, T a, T b) const { return c.G(posi, j, u, a, b); }
    double llr(int row, int pos, T s) const { return c.Q(row, pos, s); }
    bool bad() const { return false; }
};

enum Quant { Q_NONE = 0, Q_UNIFORM = 1, Q_LLOYD = 2 };

// How often the re-quantizers met the edges of their cells since the last orc_float_edge_counts: the
// clip comparison with |x| == M and the quotient x / r an integer (uniform), a probe b[mid] == x (Lloyd),
// and the first / last cell taken (uniform: the negative / positive clip).  Counted for the tests that
// show their inputs reach these edges (tests/test_float_oracle_masks_quant.py); not thread-safe.
struct EdgeCounts {
    int64_t clip_equal, quotient_integral, bisect_equal, first_cell, last_cell;
};
EdgeCounts g_edges = {0, 0, 0, 0, 0};

struct FloatDom {
    using T = double;
    int quant = Q_NONE;
    int v = 0;
    const double *r_f = nullptr, *r_g = nullptr;  // uniform step per node_posi
    // Lloyd: table t (0 = f, 1 = g) of node p is bnd[bnd_off[t*(N-1)+p] ...
    // + bnd_len[...]) and rec[rec_off[...] ... + rec_len[...])
    const double *bnd = nullptr, *rec = nullptr;
    const int32_t *bnd_off = nullptr, *bnd_len = nullptr, *rec_off = nullptr, *rec_len = nullptr;
    int nodes = 0;
    mutable bool ub = false;  // a Lloyd index outside the reconstruction (reference UB)

    static double Q(double x, double r, double M) {  // utils.cpp:8-10
        const double q = x / r;
        g_edges.clip_equal += std::fabs(x) == M;
        if (std::fabs(x) > M) {
            ++(x < 0 ? g_edges.first_cell : g_edges.last_cell);
        } else {
            g_edges.quotient_integral += q == std::floor(q);
        }
        return std::fabs(x) > M ? sgn(x) * (M - 0.5 * r) : (std::floor(x / r) + 0.5) * r;
    }
    double bisect(double a, int t, int posi) const {  // utils.cpp:12-24
        const double *b = bnd + bnd_off[t * nodes + posi];
        int lo = 0, hi = bnd_len[t * nodes + posi];
        while (lo < hi) {
            int mid = (lo + hi) / 2;
            g_edges.bisect_equal += b[mid] == a;
            if (b[mid] < a)
                lo = mid + 1;
            else
                hi = mid;
        }
        if (lo - 1 < 0 || lo - 1 >= rec_len[t * nodes + posi]) {
            ub = true;
            return 0.0;
        }
        g_edges.first_cell += lo - 1 == 0;
        g_edges.last_cell += lo - 1 == rec_len[t * nodes + posi] - 1;
        return rec[rec_off[t * nodes + posi] + lo - 1];
    }
    T f(int posi, int, T a, T b) const {
        const double x = (sgn(a) * sgn(b)) * std::min(std::fabs(a), std::fabs(b));
        if (quant == Q_UNIFORM) return Q(x, r_f[posi], double(v / 2 - 0.5) * r_f[posi]);
        if (quant == Q_LLOYD) return bisect(x, 0, posi);
        return x;
    }
    T g(int posi, int, int u, T a, T b) const {
        const double x = (1 - 2 * u) * a + b;
        if (quant == Q_UNIFORM) return Q(x, r_g[posi], double(v / 2 - 1) * r_g[posi]);
        if (quant == Q_LLOYD) return bisect(x, 1, posi);
        return x;
    }
    double llr(int, int, T s) const { return s; }
    bool bad() const { return ub; }
};

// ---------------------------------------------------------------------------
// SC family: SC (SCDecoder.cpp:14-89), SC-LUT (SCLUTDecoder.cpp:21-124),
// SC uniform/Lloyd (SCUniformQuantizedDecoder.cpp:20-99,
// SCLloydQuantizedDecoder.cpp:22-101), and with `fast` FastSC-LUT
// (FastSCLUT.cpp:27-206) / FastSC (FastSCDecoder.cpp:21-174).
// ---------------------------------------------------------------------------
template <class D>
struct SCDec {
    using T = typename D::T;
    const Code &c;
    const D &dom;
    bool fast;
    std::vector<T> sym;
    std::vector<uint8_t> ucap;
    SCDec(const Code &c_, const D &dom_, bool fast_)
        : c(c_), dom(dom_), fast(fast_), sym((c_.n + 1) * c_.N), ucap((c_.n + 1) * c_.N) {}

    // Leaf decision from a node at depth n-1 (SCLUTDecoder.cpp:59-66, 90-97;
    // SCDecoder.cpp:24-29).  Hazard H4: SC family decides `llr <= 0`.
    // Frozen leaves are 0 whatever the LLR.
    void leaf(int posi, int k, bool right, const T *pa, const T *pb, int ul) {
        const int N = c.N, n = c.n;
        if (c.frozen[k] == 1) { ucap[n * N + k] = 0; return; }
        T s = right ? dom.g(posi, 0, ul, pa[0], pb[0]) : dom.f(posi, 0, pa[0], pb[0]);
        ucap[n * N + k] = (uint8_t)(dom.llr(n - 1, k, s) <= 0);
    }

    // Special nodes, FastSCLUT.cpp:46-107 / FastSCDecoder.cpp:45-106.  LUT
    // domain: vcl row depth-1 (H3).
    bool special(int d, int node) {
        const int N = c.N;
        const int posi = (1 << d) + node - 1;
        const int t = c.type(posi);
        if (!fast || t < 0 || t > 3) return false;
        const int temp = N >> d;
        const T *ps = &sym[d * N + temp * node];
        uint8_t *pu = &ucap[d * N + temp * node];
        if (t == 0) {  // R0, :46-54
            std::memset(pu, 0, temp);
        } else if (t == 1) {  // R1, :55-66
            for (int i = 0; i < temp; ++i) pu[i] = dom.llr(d - 1, temp * node + i, ps[i]) <= 0;
        } else if (t == 2) {  // REP, :67-80 (sequential fp64 sum, H5)
            double S = 0;
            for (int i = 0; i < temp; ++i) S += dom.llr(d - 1, temp * node + i, ps[i]);
            std::memset(pu, (uint8_t)(S <= 0), temp);
        } else {  // SPC, :81-107 (first-min flip, H6)
            std::vector<double> mag(temp);
            int parity = 0;
            for (int i = 0; i < temp; ++i) {
                double l = dom.llr(d - 1, temp * node + i, ps[i]);
                pu[i] = (uint8_t)(l <= 0);
                parity += pu[i];
                mag[i] = std::fabs(l);
            }
            if (parity % 2) {
                int m = first_argmin(mag);
                pu[m] = 1 - pu[m];
            }
        }
        return true;
    }

    void visit(int d, int node) {
        const int N = c.N, n = c.n;
        if (special(d, node)) return;
        const int posi = (1 << d) + node - 1;
        const int temp = N >> d, half = temp / 2;
        const T *pa = &sym[d * N + temp * node];
        const T *pb = pa + half;
        const int l = 2 * node, r = 2 * node + 1;
        if (d + 1 < n) {
            T *lo = &sym[(d + 1) * N + half * l];
            for (int j = 0; j < half; ++j) lo[j] = dom.f(posi, j, pa[j], pb[j]);
            visit(d + 1, l);
        } else {
            leaf(posi, l, false, pa, pb, 0);
        }
        const uint8_t *ul = &ucap[(d + 1) * N + half * l];
        if (d + 1 < n) {
            T *hi = &sym[(d + 1) * N + half * r];
            for (int j = 0; j < half; ++j) hi[j] = dom.g(posi, j, ul[j], pa[j], pb[j]);
            visit(d + 1, r);
        } else {
            leaf(posi, r, true, pa, pb, ul[0]);
        }
        combine(&ucap[d * N + temp * node], ul, &ucap[(d + 1) * N + half * r], half);
    }

    template <class In>
    int run(const In *y, uint8_t *out) {
        const int N = c.N, n = c.n;
        if (fast && c.type(0) >= 0 && c.type(0) <= 3) return -2;  // reference UB (root special)
        for (int i = 0; i < N; ++i) sym[i] = (T)y[i];
        visit(0, 0);
        if (dom.bad()) return -4;
        if (!fast) {
            emit_info(c, &ucap[n * N], out);  // SCLUTDecoder.cpp:116-123
        } else {
            std::vector<uint8_t> x(ucap.begin(), ucap.begin() + N);  // FastSCLUT.cpp:186-205
            reencode(x, N);
            emit_info(c, x.data(), out);
        }
        return 0;
    }
};

// ---------------------------------------------------------------------------
// SCL family: SCL-LUT (SCLLUTDecoder.cpp:47-253), SCL (SCLDecoder.cpp:38-176),
// SCL uniform/Lloyd (SCLUniformQuantizedDecoder.cpp:43-184,
// SCLLloydQuantizedDecoder.cpp:46-187), CA-SCL (CASCLDecoder.cpp:74-249), and
// with `fast` FastSCL-LUT (FastSCLLUTDecoder.cpp:57-408) / FastSCL
// (FastSCLDecoder.cpp:49-423).  State is L full copies of the node values and
// partial sums, deep-copied at every fork exactly as the reference does.
// ---------------------------------------------------------------------------
template <class D>
struct SCLDec {
    using T = typename D::T;
    const Code &c;
    const D &dom;
    bool fast;
    int L;
    double pm_init = kInf;  // DOUBLE_INF: 1.0/0.0 (LUT kinds, FastSCL), 1e300 (SCLDecoder.h:8 ...)
    // Per path and depth d: the symbols of the node on the current descent (N >> d of them) and the
    // partial sums of the last left (0) and right (1) node finished at that depth.  The reference
    // keeps an (n + 1) x N array of each per path and copies all of it at every fork; every op writes
    // a node's block whole, so a fork that copies the blocks' handles leaves each path the same
    // contents at a cost that does not grow with N (N = 65536: minutes per frame otherwise).
    template <class X>
    using Block = std::shared_ptr<std::vector<X>>;
    struct Path {
        std::vector<Block<T>> S;
        std::vector<Block<uint8_t>> U;  // [2 * d + (node & 1)]
    };
    std::vector<Path> path;
    std::vector<double> pm;
    const T *S(int i, int d) const { return path[i].S[d]->data(); }
    const uint8_t *U(int i, int d, int node) const { return path[i].U[2 * d + (node & 1)]->data(); }
    T *new_S(int i, int d) { return (path[i].S[d] = std::make_shared<std::vector<T>>(c.N >> d))->data(); }
    uint8_t *new_U(int i, int d, int node) {
        return (path[i].U[2 * d + (node & 1)] = std::make_shared<std::vector<uint8_t>>(c.N >> d))->data();
    }

    CaSpec ca;  // ca.A > 0: CRC-aided output of A bits

    SCLDec(const Code &c_, const D &dom_, bool fast_) : c(c_), dom(dom_), fast(fast_), L(c_.L) {}

    // Keep L survivors of the 2L candidates `pm2` (mink, :8-21).  Returns the
    // parent path and whether the candidate came from the upper half.
    void select(const std::vector<double> &pm2, std::vector<int> &parent, std::vector<bool> &upper) {
        std::vector<int> order = sort_index(pm2);
        parent.assign(L, 0);
        upper.assign(L, false);
        for (int i = 0; i < L; ++i) {
            pm[i] = pm2[order[i]];
            upper[i] = order[i] >= L;
            parent[i] = upper[i] ? order[i] - L : order[i];
        }
    }
    void permute(const std::vector<int> &parent) {
        std::vector<Path> p2(L);
        for (int i = 0; i < L; ++i) p2[i] = path[parent[i]];
        path.swap(p2);
    }

    // Leaf k from a node at depth n-1 (left :91-145, right :166-221).
    // H3: vcl row n-1.  H4: decisions `DM < 0`.
    void leaf(int posi, int d, int node, int k, bool right) {
        const int N = c.N, n = c.n;
        const int temp = N >> d, half = temp / 2;
        std::vector<double> dm(L);
        for (int i = 0; i < L; ++i) {
            const T *p = S(i, d);
            T s = right ? dom.g(posi, 0, U(i, d + 1, 2 * node)[0], p[0], p[half])
                        : dom.f(posi, 0, p[0], p[half]);
            dm[i] = dom.llr(n - 1, k, s);
        }
        if (c.frozen[k] == 1) {
            for (int i = 0; i < L; ++i) {
                new_U(i, n, k)[0] = 0;
                pm[i] += std::fabs(dm[i]) * (double)(dm[i] < 0);
            }
            return;
        }
        std::vector<double> pm2(2 * L);
        std::vector<uint8_t> dec(L);
        for (int i = 0; i < L; ++i) {
            pm2[i] = pm[i];
            pm2[i + L] = pm[i] + std::fabs(dm[i]);
            dec[i] = (uint8_t)(dm[i] < 0);
        }
        std::vector<int> parent;
        std::vector<bool> upper;
        select(pm2, parent, upper);
        permute(parent);
        for (int i = 0; i < L; ++i) {
            uint8_t b = dec[parent[i]];
            new_U(i, n, k)[0] = upper[i] ? (uint8_t)(1 - b) : b;
        }
    }

    // FastSCL special nodes, FastSCLLUTDecoder.cpp:82-213 /
    // FastSCLDecoder.cpp:122-251.  SPC (type 3) has no handler in either
    // reference (LUT :215 TODO; float :253-345 commented out) and falls
    // through (H7).
    bool special(int d, int node) {
        const int N = c.N;
        const int posi = (1 << d) + node - 1;
        const int t = c.type(posi);
        if (!fast || t < 0 || t > 2) return false;
        const int temp = N >> d;
        if (t == 0) {  // R0, :83-96
            for (int i = 0; i < L; ++i) {
                new_U(i, d, node);  // zeros
                for (int j = 0; j < temp; ++j) {
                    double l = dom.llr(d - 1, temp * node + j, S(i, d)[j]);
                    pm[i] += (float)(l < 0) * std::fabs(l);
                }
            }
        } else if (t == 1) {  // R1, :99-166
            const int depth = std::min(L - 1, temp);
            std::vector<std::vector<uint8_t>> dec(L, std::vector<uint8_t>(temp));
            std::vector<std::vector<double>> mag(L, std::vector<double>(temp));
            std::vector<std::vector<int>> order(L);
            for (int i = 0; i < L; ++i) {
                for (int j = 0; j < temp; ++j) {
                    double l = dom.llr(d - 1, temp * node + j, S(i, d)[j]);
                    dec[i][j] = (uint8_t)(l < 0);
                    mag[i][j] = std::fabs(l);
                }
                order[i] = sort_index(mag[i]);
            }
            for (int layer = 0; layer < depth; ++layer) {
                std::vector<double> pm2(2 * L);
                for (int i = 0; i < L; ++i) {
                    pm2[i] = pm[i];
                    pm2[i + L] = pm[i] + mag[i][order[i][layer]];
                }
                std::vector<int> parent;
                std::vector<bool> upper;
                select(pm2, parent, upper);
                std::vector<std::vector<uint8_t>> dec2(L);
                std::vector<std::vector<double>> mag2(L);
                std::vector<std::vector<int>> order2(L);
                for (int i = 0; i < L; ++i) {
                    dec2[i] = dec[parent[i]];
                    // H2: the flipped position comes from slot i's own (pre-
                    // permutation) order, not from the parent's (:145).
                    if (upper[i]) {
                        int q = order[i][layer];
                        dec2[i][q] = 1 - dec2[i][q];
                    }
                    mag2[i] = mag[parent[i]];
                    order2[i] = order[parent[i]];
                }
                permute(parent);
                dec.swap(dec2);
                mag.swap(mag2);
                order.swap(order2);
            }
            for (int i = 0; i < L; ++i) std::memcpy(new_U(i, d, node), dec[i].data(), temp);
        } else {  // REP, :169-213
            std::vector<double> pm2(2 * L);
            for (int i = 0; i < L; ++i) {
                pm2[i] = pm[i];
                pm2[i + L] = pm[i];
            }
            for (int i = 0; i < L; ++i) {
                for (int j = 0; j < temp; ++j) {
                    double l = dom.llr(d - 1, temp * node + j, S(i, d)[j]);
                    pm2[i] += (double)(l < 0) * std::fabs(l);
                    pm2[i + L] += (double)(l >= 0) * std::fabs(l);
                }
            }
            std::vector<int> parent;
            std::vector<bool> upper;
            select(pm2, parent, upper);
            permute(parent);
            for (int i = 0; i < L; ++i) std::memset(new_U(i, d, node), upper[i] ? 1 : 0, temp);
        }
        return true;
    }

    void visit(int d, int node) {
        const int N = c.N, n = c.n;
        if (special(d, node)) return;
        const int posi = (1 << d) + node - 1;
        const int temp = N >> d, half = temp / 2;
        const int l = 2 * node, r = 2 * node + 1;
        // f (:83-90 / :223-230)
        if (d + 1 < n) {
            for (int i = 0; i < L; ++i) {
                const T *s = S(i, d);
                T *o = new_S(i, d + 1);
                for (int j = 0; j < half; ++j) o[j] = dom.f(posi, j, s[j], s[half + j]);
            }
            visit(d + 1, l);
        } else {
            leaf(posi, d, node, l, false);
        }
        // g (:157-165 / :297-305)
        if (d + 1 < n) {
            for (int i = 0; i < L; ++i) {
                const T *s = S(i, d);
                const uint8_t *ul = U(i, d + 1, l);
                T *o = new_S(i, d + 1);
                for (int j = 0; j < half; ++j) o[j] = dom.g(posi, j, ul[j], s[j], s[half + j]);
            }
            visit(d + 1, r);
        } else {
            leaf(posi, d, node, r, true);
        }
        // combine (:226-241 / :366-384)
        for (int i = 0; i < L; ++i) {
            const Block<uint8_t> ul = path[i].U[2 * (d + 1)], ur = path[i].U[2 * (d + 1) + 1];
            combine(new_U(i, d, node), ul->data(), ur->data(), half);
        }
    }

    template <class In>
    int run(const In *y, uint8_t *out, Status *st = nullptr) {
        const int N = c.N, n = c.n;
        if (fast && c.type(0) >= 0 && c.type(0) <= 2) return -2;  // reference UB (root special)
        path.assign(L, Path{std::vector<Block<T>>(n + 1), std::vector<Block<uint8_t>>(2 * (n + 1))});
        pm.assign(L, pm_init);
        pm[0] = 0;
        for (int i = 0; i < L; ++i) {
            T *s = new_S(i, 0);
            for (int k = 0; k < N; ++k) s[k] = (T)y[k];
        }
        visit(0, 0);
        if (dom.bad()) return -4;
        for (double p : pm)
            if (std::isnan(p)) return -4;  // NaN keys: std::sort's order is undefined
        std::vector<uint8_t> info = epilogue(st);
        std::memcpy(out, info.data(), info.size());
        return 0;
    }

    // Decoded info bits of a path: the leaf decisions (SCL, :244-252 / :268-275) or the re-encoded root
    // partial sums (FastSCL, :338-355 / :387-406) -- the same bits, the combines being the polar
    // transform and the transform its own inverse.
    std::vector<uint8_t> info_of(int pth) const {
        std::vector<uint8_t> x(U(pth, 0, 0), U(pth, 0, 0) + c.N);
        reencode(x, c.N);
        std::vector<uint8_t> info(c.K);
        emit_info(c, x.data(), info.data());
        return info;
    }

    // The one output stage of every list kind: the output path, its bits, and (st) what the reference
    // computes beside them and drops.  No CRC: the first minimum of PML (H6).  CRC-aided
    // (CASCLLUTDecoder.cpp:263-302, CASCLDecoder.cpp:202-235): the first path in argsort(PML) order
    // whose check code, the mask XORed onto its tail (CASCLWithRNTI.cpp:222-224), equals the nchk
    // bits after the A info bits; else the first in that order.
    std::vector<uint8_t> epilogue(Status *st) const {
        int winner = first_argmin(pm);
        bool passed = false;
        std::vector<uint8_t> info;
        if (ca.A > 0) {
            std::vector<int> order = sort_index(pm);
            winner = order[0];
            for (int i = 0; i < L && !passed; ++i) {
                info = info_of(order[i]);
                std::vector<uint8_t> head(info.begin(), info.begin() + ca.A);
                std::vector<uint8_t> chk = crc_encoding(head, ca.crc_n, ca.p);
                const int m = (int)ca.mask.size();
                for (int l = 0; l < m; ++l) chk[ca.crc_n - m + l] ^= ca.mask[l];
                passed = std::equal(chk.begin(), chk.begin() + ca.nchk, info.begin() + ca.A);
                if (passed) winner = order[i];
            }
        }
        if (!passed) info = info_of(winner);
        if (ca.A > 0) info.resize(ca.A);
        if (st) {
            st->pml = pm;
            st->winner = winner;
            st->passed = passed;
        }
        return info;
    }
};

Code make_code(int32_t N, int32_t K, int32_t L, int32_t v, const int32_t *frozen, const int32_t *node_type,
               const uint8_t *lut_f, const int32_t *f_base, int32_t f_step, const uint8_t *lut_g,
               const int32_t *g_base, int32_t g_step, const double *vcl, int32_t vcl_rows) {
    Code c;
    c.N = N;
    c.K = K;
    c.L = L;
    c.v = v;
    c.n = ilog2(N);
    c.frozen = frozen;
    c.node_type = node_type;
    c.lut_f = lut_f;
    c.f_base = f_base;
    c.f_step = f_step;
    c.lut_g = lut_g;
    c.g_base = g_base;
    c.g_step = g_step;
    c.vcl = vcl;
    c.vcl_rows = vcl_rows;
    return c;
}

// CRC of a CRC-aided decode; false for a mask that is longer than the check code or not of 0 / 1.
bool set_crc(CaSpec &ca, int A, int crc_n, int nchk, const int32_t *crc_loc, int n_loc, const uint8_t *mask,
             int mask_bits) {
    if (mask_bits < 0 || mask_bits > crc_n) return false;
    ca.A = A;
    ca.crc_n = crc_n;
    ca.nchk = nchk;
    ca.p.assign(crc_n + 1, 0);
    for (int i = 0; i < n_loc; ++i) ca.p[crc_loc[i]] = 1;
    ca.mask.assign(mask, mask + mask_bits);
    for (uint8_t m : ca.mask)
        if (m > 1) return false;
    return true;
}

// Frames [0, B) through a list decoder; pml [B][L], winner [B], passed [B] where asked for.
template <class D, class In>
int decode_list(SCLDec<D> &dec, const In *in, int N, int64_t B, uint8_t *out, int ob, double *pml, int32_t *winner,
                uint8_t *passed) {
    Status st;
    for (int64_t b = 0; b < B; ++b) {
        int rc = dec.run(in + b * N, out + b * ob, &st);
        if (rc) return rc;
        if (pml) std::copy(st.pml.begin(), st.pml.end(), pml + b * dec.L);
        if (winner) winner[b] = st.winner;
        if (passed) passed[b] = st.passed;
    }
    return 0;
}

}  // namespace

extern "C" {

// List kinds with status: kind 2 = SCL-LUT / CA-SCL-LUT, 4 = FastSCL-LUT / CA-FastSCL-LUT; A == 0: no CRC
// (out uint8 [B][K]), else the CRC-aided decoder (out [B][A]; crc_loc lists the nonzero coefficient
// indices, CRC::CRC, utils.cpp:69-75).  mask: mask_bits entries of 0 / 1, entry l XORed onto check-code
// bit crc_n - mask_bits + l before the compare (CASCLWithRNTI.cpp:222-224).  pml [B][L]: every path's final
// metric in path-index order; winner [B]: the output path's index; passed [B]: its CRC compare
// succeeded (0 without CRC).  Each of the three may be null.
int orc_decode_lut_status(int32_t kind, int32_t N, int32_t K, int32_t A, int32_t L, int32_t v, const int32_t *frozen,
                          const int32_t *node_type, const uint8_t *lut_f, const int32_t *f_base, int32_t f_step,
                          const uint8_t *lut_g, const int32_t *g_base, int32_t g_step, const double *vcl,
                          int32_t vcl_rows, int32_t crc_n, const int32_t *crc_loc, int32_t n_loc, const uint8_t *mask,
                          int32_t mask_bits, const int32_t *sym, int64_t B, uint8_t *out, double *pml,
                          int32_t *winner, uint8_t *passed) {
    if (kind != 2 && kind != 4) return -3;
    if (A < 0 || A > K || (A > 0 && K - A > crc_n) || (A == 0 && mask_bits != 0)) return -1;
    Code c = make_code(N, K, L, v, frozen, node_type, lut_f, f_base, f_step, lut_g, g_base, g_step, vcl, vcl_rows);
    if (N < 2 || (1 << c.n) != N) return -1;
    LutDom dom{c};
    SCLDec<LutDom> dec(c, dom, kind == 4);
    if (A > 0 && !set_crc(dec.ca, A, crc_n, K - A, crc_loc, n_loc, mask, mask_bits)) return -1;
    return decode_list(dec, sym, N, B, out, A > 0 ? A : K, pml, winner, passed);
}

// kind: 1 = SC-LUT, 2 = SCL-LUT, 3 = FastSC-LUT, 4 = FastSCL-LUT.
// Decodes frames [0, B) of `sym` (int32 [B][N]) into `out` (uint8 [B][K]).
int orc_decode_lut(int32_t kind, int32_t N, int32_t K, int32_t L, int32_t v, const int32_t *frozen,
                   const int32_t *node_type, const uint8_t *lut_f, const int32_t *f_base, int32_t f_step,
                   const uint8_t *lut_g, const int32_t *g_base, int32_t g_step, const double *vcl,
                   int32_t vcl_rows, const int32_t *sym, int64_t B, uint8_t *out) {
    if (kind == 2 || kind == 4)
        return orc_decode_lut_status(kind, N, K, 0, L, v, frozen, node_type, lut_f, f_base, f_step, lut_g, g_base,
                                     g_step, vcl, vcl_rows, 0, nullptr, 0, nullptr, 0, sym, B, out, nullptr, nullptr,
                                     nullptr);
    if (kind != 1 && kind != 3) return -3;
    Code c = make_code(N, K, 1, v, frozen, node_type, lut_f, f_base, f_step, lut_g, g_base, g_step, vcl, vcl_rows);
    if (N < 2 || (1 << c.n) != N) return -1;
    LutDom dom{c};
    SCDec<LutDom> dec(c, dom, kind == 3);
    for (int64_t b = 0; b < B; ++b) {
        int rc = dec.run(sym + b * N, out + b * K);
        if (rc) return rc;
    }
    return 0;
}

// CRC-aided list decoders: kind 2 = CA-SCL-LUT, 4 = CA-FastSCL-LUT (the
// list kinds above plus the CRC epilogue).  Output uint8 [B][A].
int orc_decode_lut_ca(int32_t kind, int32_t N, int32_t K, int32_t A, int32_t L, int32_t v, const int32_t *frozen,
                      const int32_t *node_type, const uint8_t *lut_f, const int32_t *f_base, int32_t f_step,
                      const uint8_t *lut_g, const int32_t *g_base, int32_t g_step, const double *vcl,
                      int32_t vcl_rows, int32_t crc_n, const int32_t *crc_loc, int32_t n_loc, const int32_t *sym,
                      int64_t B, uint8_t *out) {
    if (kind != 2 && kind != 4) return -3;
    if (A < 1) return -1;
    return orc_decode_lut_status(kind, N, K, A, L, v, frozen, node_type, lut_f, f_base, f_step, lut_g, g_base, g_step,
                                 vcl, vcl_rows, crc_n, crc_loc, n_loc, nullptr, 0, sym, B, out, nullptr, nullptr,
                                 nullptr);
}

// Float SC (min-sum), SCDecoder.cpp:14-89.  llr is float64 [B][N].
int orc_decode_sc_float(int32_t N, int32_t K, const int32_t *frozen, const double *llr, int64_t B, uint8_t *out) {
    Code c = make_code(N, K, 1, 1, frozen, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, nullptr, 0);
    if (N < 2 || (1 << c.n) != N) return -1;
    FloatDom dom;
    SCDec<FloatDom> dec(c, dom, false);
    for (int64_t b = 0; b < B; ++b) dec.run(llr + b * N, out + b * K);
    return 0;
}

// Float-domain decoders on float64 LLRs [B][N] (kinds as include/qpd.h):
//   0 SC            SCDecoder.cpp:14-89
//   7 SCL           SCLDecoder.cpp:38-176              (PM init 1e300, SCLDecoder.h:8)
//   8 CA-SCL        CASCLDecoder.cpp:74-249            (1e300; CRC from crc_n/crc_loc,
//                                                       crc_n bits compared, :202-235)
//   9 FastSC        FastSCDecoder.cpp:21-174
//  10 FastSCL       FastSCLDecoder.cpp:49-423          (PM init 1.0/0.0, FastSCLDecoder.h:7)
//  11 SC-Uniform    SCUniformQuantizedDecoder.cpp:20-99
//  12 SCL-Uniform   SCLUniformQuantizedDecoder.cpp:43-184 (1e300)
//  13 SC-Lloyd      SCLloydQuantizedDecoder.cpp:22-101
//  14 SCL-Lloyd     SCLLloydQuantizedDecoder.cpp:46-187   (1e300)
// Output uint8 [B][K] ([B][A] for kind 8).  Returns -4 where the reference's
// behaviour is undefined (Lloyd index outside the reconstruction, NaN path
// metrics).
// With status (list kinds; mask, pml, winner, passed as orc_decode_lut_status, the mask for kind 8 only):
// each of pml, winner, passed may be null, and all are for the SC kinds.
int orc_decode_float_status(int32_t kind, int32_t N, int32_t K, int32_t L, const int32_t *frozen,
                            const int32_t *node_type, int32_t v, const double *r_f, const double *r_g, const double *bnd,
                            const int32_t *bnd_off, const int32_t *bnd_len, const double *rec, const int32_t *rec_off,
                            const int32_t *rec_len, int32_t A, int32_t crc_n, const int32_t *crc_loc, int32_t n_loc,
                            const uint8_t *mask, int32_t mask_bits, const double *llr, int64_t B, uint8_t *out,
                            double *pml, int32_t *winner, uint8_t *passed) {
    const bool list = kind == 7 || kind == 8 || kind == 10 || kind == 12 || kind == 14;
    const bool fast = kind == 9 || kind == 10;
    Code c = make_code(N, K, list ? L : 1, v, frozen, fast ? node_type : nullptr, nullptr, nullptr, 0, nullptr,
                       nullptr, 0, nullptr, 0);
    if (N < 2 || (1 << c.n) != N) return -1;
    FloatDom dom;
    dom.v = v;
    dom.nodes = N - 1;
    if (kind == 11 || kind == 12) {
        dom.quant = Q_UNIFORM;
        dom.r_f = r_f;
        dom.r_g = r_g;
    } else if (kind == 13 || kind == 14) {
        dom.quant = Q_LLOYD;
        dom.bnd = bnd;
        dom.bnd_off = bnd_off;
        dom.bnd_len = bnd_len;
        dom.rec = rec;
        dom.rec_off = rec_off;
        dom.rec_len = rec_len;
    } else if (kind != 0 && kind != 7 && kind != 8 && kind != 9 && kind != 10) {
        return -3;
    }
    if (kind != 8 && mask_bits != 0) return -1;
    if (!list) {
        if (pml || winner || passed) return -1;
        SCDec<FloatDom> dec(c, dom, fast);
        for (int64_t b = 0; b < B; ++b) {
            int rc = dec.run(llr + b * N, out + b * K);
            if (rc) return rc;
        }
        return 0;
    }
    SCLDec<FloatDom> dec(c, dom, fast);
    dec.pm_init = kind == 10 ? kInf : 1e300;
    if (kind == 8) {
        if (A < 1 || crc_n < 1 || A + crc_n > K) return -1;
        if (!set_crc(dec.ca, A, crc_n, crc_n, crc_loc, n_loc, mask, mask_bits)) return -1;
    }
    return decode_list(dec, llr, N, B, out, kind == 8 ? A : K, pml, winner, passed);
}

// Copies the five counters of EdgeCounts (in its order) to out and clears them.
void orc_float_edge_counts(int64_t *out) {
    const int64_t v[5] = {g_edges.clip_equal, g_edges.quotient_integral, g_edges.bisect_equal, g_edges.first_cell,
                          g_edges.last_cell};
    for (int i = 0; i < 5; ++i) out[i] = v[i];
    g_edges = EdgeCounts{0, 0, 0, 0, 0};
}

int orc_decode_float(int32_t kind, int32_t N, int32_t K, int32_t L, const int32_t *frozen, const int32_t *node_type,
                     int32_t v, const double *r_f, const double *r_g, const double *bnd, const int32_t *bnd_off,
                     const int32_t *bnd_len, const double *rec, const int32_t *rec_off, const int32_t *rec_len,
                     int32_t A, int32_t crc_n, const int32_t *crc_loc, int32_t n_loc, const double *llr, int64_t B,
                     uint8_t *out) {
    return orc_decode_float_status(kind, N, K, L, frozen, node_type, v, r_f, r_g, bnd, bnd_off, bnd_len, rec, rec_off,
                                   rec_len, A, crc_n, crc_loc, n_loc, nullptr, 0, llr, B, out, nullptr, nullptr, nullptr);
}

}  // extern "C"
