// Test harness (CPU): the transmit side's host code without a device -- the argument
// rules (qpd_tx.hpp: check_encode, check_frames) and the host encoder (encode_host)
// exactly as qpd_capi.hip calls them, and for the round trips the host engine behind
// them.  A program of its own, built with g++ beside the tests from the library's sources:
//     tx_harness CASE RESULT
// CASE (little endian): int32 h[24] =
//     mode (0 encode, 1 the checks of qpd_tx_frames, 2 encode -> LLR -+20 -> host-engine decode),
//     kind, N, K, A, crc_n, crc_loc_count, B, mask_bits (-1: tx = NULL), null_mask, want_info,
//     want_cw, no_signal, null_msg, out_type, has_ch, q, has_rec, null_frames, frames_offset,
//     frame0, L, dec_mask_bits, has_node_type;
// int32 frozen[N]; int32 crc_loc[crc_loc_count]; uint8 mask[max(mask_bits, 0)];
// uint8 dec_mask[dec_mask_bits]; uint8 msg[B][A'] (A' = A for the CRC-aided kinds, else K);
// int32 node_type[2N-1] (has_node_type).
// RESULT: int32 rc (QPD_E_*; 99: a byte outside the B rows was written), int32 flag
// (qpd::ErrFlag of the encoder), then for rc == 0: mode 0: info[B][K] (want_info),
// codeword[B][N] (want_cw); mode 2: bits[B][A'], pass[B].  A refusal's message goes to stdout.
#include <cstdio>
#include <memory>
#include <vector>

#include "qpd_config.hpp"
#include "qpd_status.hpp"
#include "qpd_tx.hpp"

template <class T>
static bool get(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

static const uint8_t kSentinel = 0xA5;

// rows * width bytes with one sentinel row in front and one behind
struct Guarded {
    std::vector<uint8_t> buf;
    size_t width, rows;
    Guarded(size_t rows_, size_t width_) : buf((rows_ + 2) * width_ + 2, kSentinel), width(width_), rows(rows_) {}
    uint8_t *data() { return buf.data() + width + 1; }
    bool intact() const {
        for (size_t i = 0; i < width + 1; ++i)
            if (buf[i] != kSentinel || buf[buf.size() - 1 - i] != kSentinel) return false;
        return true;
    }
};

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<int32_t> h, frozen, crc_loc, node_type;
    std::vector<uint8_t> mask, dec_mask, msg;
    if (!get(in, h, 24)) return 2;
    const int mode = h[0], kind = h[1], N = h[2], K = h[3], A = h[4], crc_n = h[5], nloc = h[6];
    const int64_t B = h[7];
    const int mask_bits = h[8], L = h[21], dec_mask_bits = h[22];
    if (N < 1 || N > 65536 || K < 0 || K > N || nloc < 0 || nloc > 64 || B < -1 || B > (1 << 20)) return 2;
    const bool ca = qpd_sched::is_ca(kind);
    const int Am = ca ? A : K;
    if (!get(in, frozen, (size_t)N) || !get(in, crc_loc, (size_t)nloc) || !get(in, mask, (size_t)(mask_bits > 0 ? mask_bits : 0)) ||
        !get(in, dec_mask, (size_t)dec_mask_bits) || !get(in, msg, (size_t)(B > 0 ? B : 0) * Am))
        return 2;
    if (h[23] && !get(in, node_type, (size_t)2 * N - 1)) return 2;
    fclose(in);

    qpd_tx_args tx{};
    tx.crc_mask = h[9] ? nullptr : mask.data();
    tx.crc_mask_bits = mask_bits == -1 ? 0 : mask_bits;
    tx.no_signal = h[12];
    const qpd_tx_args *txp = mask_bits == -1 ? nullptr : &tx;
    const uint8_t *msgp = h[13] ? nullptr : msg.data();
    const int cfg_crc_n = ca ? crc_n : 0;

    std::string err;
    uint32_t mword = 0;
    bool run = false;
    int32_t rc = 0, flag = 0;
    Guarded info(h[10] ? (size_t)(B > 0 ? B : 0) : 0, (size_t)K), cw(h[11] ? (size_t)(B > 0 ? B : 0) : 0, (size_t)N);
    std::vector<uint8_t> bits, pass;
    if (mode == 1) {
        static double frames[4];
        const void *fp = h[18] ? nullptr : (const void *)((const char *)frames + h[19]);
        rc = qpd_tx::check_frames(kind, K, A, cfg_crc_n, txp, h[20], B, msgp, h[14], h[15] != 0, h[16], h[17] != 0, fp, &mword, &run,
                                  err);
    } else {
        rc = qpd_tx::check_encode(kind, K, A, cfg_crc_n, txp, B, msgp, h[10] ? info.data() : nullptr, h[11] ? cw.data() : nullptr,
                                  &mword, &run, err);
        if (!rc && run) {
            const uint32_t q = ca ? qpd_cfg::crc_taps(crc_n, crc_loc.data(), nloc) : 0u;
            const qpd_tx::Code code = qpd_tx::make_code(N, K, A, cfg_crc_n, q, frozen.data());
            flag = qpd_tx::encode_host(code, msgp, B, mword, h[10] ? info.data() : nullptr, h[11] ? cw.data() : nullptr);
            if (!info.intact() || !cw.intact()) rc = 99;
        }
    }
    if (!rc && mode == 2 && run) {
        qpd_config c{};
        c.kind = kind;
        c.N = N;
        c.K = K;
        c.L = L;
        c.frozen_bits = frozen.data();
        c.A = A;
        c.crc_n = cfg_crc_n;
        c.crc_loc = crc_loc.data();
        c.crc_loc_count = ca ? nloc : 0;
        if (h[23]) c.node_type = node_type.data();  // the Fast kinds' labels
        std::unique_ptr<qpd_host::Plan> p = qpd_host::make_plan(&c);
        if (!p || p->out_k != Am) return 2;
        qpd_host::Engine<double> e(*p);
        std::vector<double> llr((size_t)B * N);
        for (size_t i = 0; i < llr.size(); ++i) llr[i] = cw.data()[i] ? -20.0 : 20.0;
        bits.assign((size_t)B * Am, 7);
        pass.assign((size_t)B, 7);
        qpd_status_args sa{};
        sa.crc_mask = dec_mask.data();
        sa.crc_mask_bits = dec_mask_bits;
        sa.crc_pass = ca ? pass.data() : nullptr;
        qpd_stat::Req rq;
        rc = qpd_stat::check(kind, L, cfg_crc_n, QPD_IN_F64, &sa, &rq, err);
        if (!rc) rc = qpd_stat::host_run(&e, llr.data(), B, N, p->out_k, bits.data(), rq);
    }
    if (rc) printf("%s\n", err.c_str());
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    fwrite(&rc, sizeof(rc), 1, out);
    fwrite(&flag, sizeof(flag), 1, out);
    if (rc == 0 && mode == 0 && run) {
        if (h[10]) fwrite(info.data(), 1, (size_t)B * K, out);
        if (h[11]) fwrite(cw.data(), 1, (size_t)B * N, out);
    }
    if (rc == 0 && mode == 2) {
        fwrite(bits.data(), 1, bits.size(), out);
        fwrite(pass.data(), 1, pass.size(), out);
    }
    fclose(out);
    return 0;
}
