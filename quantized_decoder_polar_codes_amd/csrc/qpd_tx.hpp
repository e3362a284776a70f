// qpd_tx.hpp -- the transmit side's host code (qpd_encode / qpd_encode_host /
// qpd_tx_frames, qpd.h): the argument rules, the per-code constants the encoder
// needs (word-packed information mask, information bits before each word, the
// CRC register's contribution per message bit) and the host encoder.  Host code
// without HIP, as qpd_status.hpp and qpd_dmetric.hpp: the CPU tests build it into
// tests/native/tx_harness.cpp.
//
// The host encoder is the kernel's algorithm on 32-bit words (csrc/qpd_tx.hip):
// message bytes packed to bits, the CRC as a table XOR over the set message bits
// (the register is linear in them, utils.cpp:77-92), the information bits
// deposited at the mask's set positions, five in-word butterfly stages and
// log2(N / 32) word stages of x = u F^{(x)n}.  qpd_encode_host always runs it for
// host buffers, whatever the batch: there is no crossover model between it and
// the device (a host batch large enough for the GPU to win would first have to
// cross PCIe twice with one byte per bit; callers with such batches hold them on
// the device and call qpd_encode).
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "qpd.h"
#include "qpd_schedule.hpp"
#include "qpd_types.hpp"

namespace qpd_tx {

// The encoder's constants of one code.  A = K and crc_n = 0 for a kind without CRC.
struct Code {
    int N = 0, K = 0, A = 0, crc_n = 0;
    std::vector<uint32_t> info_mask;  // [ceil(N/32)] bit i of word w: position 32w+i is an information bit
    std::vector<int32_t> info_pref;   // information bits before word w
    std::vector<uint32_t> crc_tab;    // [A] CRC register after message bit j alone (crc_n > 0)
};

// mask_words: the word-packed information mask (qpd_decoder::info_mask); crc_q: the
// divisor's taps as register bits (qpd_cfg::crc_taps).
inline Code make_code(int N, int K, int A, int crc_n, uint32_t crc_q, const uint32_t *mask_words) {
    Code c;
    c.N = N;
    c.K = K;
    c.crc_n = crc_n > 0 ? crc_n : 0;
    c.A = c.crc_n ? A : K;
    const int nw = (N + 31) / 32;
    c.info_mask.assign(mask_words, mask_words + nw);
    c.info_pref.assign(nw, 0);
    for (int w = 1; w < nw; ++w) c.info_pref[w] = c.info_pref[w - 1] + __builtin_popcount(c.info_mask[w - 1]);
    // tab[A-1] = taps, tab[j] = one zero step of tab[j+1] (mc_constants, qpd_capi_mc.hpp)
    c.crc_tab.assign(c.crc_n ? c.A : 0, 0u);
    if (c.crc_n) {
        const uint32_t top = 1u << (c.crc_n - 1), msk = (top << 1) - 1u;
        c.crc_tab[c.A - 1] = crc_q & msk;
        for (int j = c.A - 2; j >= 0; --j) {
            const uint32_t r = c.crc_tab[j + 1];
            c.crc_tab[j] = ((r << 1) & msk) ^ ((r & top) ? crc_q : 0u);
        }
    }
    return c;
}

// The same from a 0/1 frozen array (qpd_config.frozen_bits; 0 = information).
inline Code make_code(int N, int K, int A, int crc_n, uint32_t crc_q, const int32_t *frozen) {
    std::vector<uint32_t> m((N + 31) / 32, 0u);
    for (int i = 0; i < N; ++i)
        if (!frozen[i]) m[i >> 5] |= 1u << (i & 31);
    return make_code(N, K, A, crc_n, crc_q, m.data());
}

// The rules every transmit call shares.  kind, K, A, crc_n: the decoder's
// (qpd_config; A and crc_n only read for the CRC-aided kinds).  tx may be NULL.
// *mask: the CRC mask as the register word the encoder XORs -- mask bit l meets
// check-code bit crc_n - bits + l, register bit bits - 1 - l, the word
// qpd_decode_status compares under (qpd_stat::check).  Returns QPD_OK or the
// refusal with its message in err.
inline int check_common(int kind, int K, int A, int crc_n, const qpd_tx_args *tx, uint32_t *mask, std::string &err) {
    auto refuse = [&](int rc, const char *msg) {
        err = msg;
        return rc;
    };
    int fam = 0, dom = 0;
    *mask = 0;
    if (!qpd_sched::family_of(kind, &fam, &dom)) return refuse(QPD_E_INVALID, "bad kind");
    const bool ca = qpd_sched::is_ca(kind);
    // the message carries K - A bits of the crc_n-bit check code; QPD_CASCL_FLOAT compares
    // crc_n of them, so it is served where A + crc_n == K (as qpd_mc_llr)
    if (ca && K - A > crc_n)
        return refuse(QPD_E_UNSUPPORTED, "a CRC-aided code needs K - A <= crc_n to be encoded (CASCLDecoder: A + crc_n == K)");
    if (!tx) return QPD_OK;
    if (tx->crc_mask_bits < 0 || tx->crc_mask_bits > (ca ? crc_n : 0))
        return refuse(QPD_E_INVALID, ca ? "crc_mask_bits must be in [0, crc_n]" : "crc_mask: not a CRC-aided decoder");
    if (tx->crc_mask_bits > 0 && !tx->crc_mask) return refuse(QPD_E_INVALID, "crc_mask is NULL with crc_mask_bits > 0");
    for (int l = 0; l < tx->crc_mask_bits; ++l) {
        if (tx->crc_mask[l] > 1) return refuse(QPD_E_INVALID, "crc_mask entries must be 0 or 1");
        *mask |= (uint32_t)tx->crc_mask[l] << (tx->crc_mask_bits - 1 - l);
    }
    return QPD_OK;
}

// qpd_encode / qpd_encode_host.  *run = false where there is nothing to do (a
// refusal, or an empty batch: QPD_OK).
inline int check_encode(int kind, int K, int A, int crc_n, const qpd_tx_args *tx, int64_t B, const void *msg,
                        const void *info, const void *codeword, uint32_t *mask, bool *run, std::string &err) {
    *run = false;
    const int rc = check_common(kind, K, A, crc_n, tx, mask, err);
    if (rc) return rc;
    if (tx && tx->no_signal) {
        err = "no_signal is qpd_tx_frames' (an encoder has no channel)";
        return QPD_E_INVALID;
    }
    if (B < 0) {
        err = "negative batch B";
        return QPD_E_INVALID;
    }
    if (!info && !codeword) {
        err = "d_info and d_codeword are both NULL: nothing to write";
        return QPD_E_INVALID;
    }
    if (B == 0) return QPD_OK;
    if (!msg) {
        err = "msg is NULL";
        return QPD_E_INVALID;
    }
    *run = true;
    return QPD_OK;
}

// qpd_tx_frames, up to the channel's own rules (check_channel / check_llr_channel,
// qpd_capi_mc.hpp, which need the quantizer's arrays): q is ch->q, has_rec whether
// rec was given.
inline int check_frames(int kind, int K, int A, int crc_n, const qpd_tx_args *tx, int64_t frame0, int64_t B,
                        const void *msg, int32_t out_type, bool has_channel, int q, bool has_rec, const void *frames,
                        uint32_t *mask, bool *run, std::string &err) {
    *run = false;
    const int rc = check_common(kind, K, A, crc_n, tx, mask, err);
    if (rc) return rc;
    auto refuse = [&](const char *msg_) {
        err = msg_;
        return QPD_E_INVALID;
    };
    if (!has_channel) return refuse("ch is NULL");
    if (out_type < QPD_TX_SYM_I32 || out_type > QPD_TX_LLR_F64)
        return refuse("out_type must be QPD_TX_SYM_I32, QPD_TX_SYM_U8 or QPD_TX_LLR_F64");
    if (has_rec && out_type != QPD_TX_LLR_F64) return refuse("rec applies to out_type QPD_TX_LLR_F64 only");
    if (out_type == QPD_TX_SYM_U8 && q > 256) return refuse("out_type QPD_TX_SYM_U8 needs q <= 256");
    if (B < 0 || frame0 < 0) return refuse("negative frame range (frame0, B)");
    if (B == 0) return QPD_OK;
    if (!frames) return refuse("d_frames is NULL");
    if (!msg && !(tx && tx->no_signal)) return refuse("d_msg is NULL (only no_signal = 1 needs no message)");
    if (out_type == QPD_TX_LLR_F64 && ((uintptr_t)frames & 7u) != 0)
        return refuse("d_frames alignment: float64 LLRs need an 8-byte aligned base");
    if (out_type == QPD_TX_SYM_I32 && ((uintptr_t)frames & 3u) != 0)
        return refuse("d_frames alignment: int32 symbols need a 4-byte aligned base");
    *run = true;
    return QPD_OK;
}

// B messages (host, [B][A] bytes) -> information bits ([B][K], or NULL) and
// codewords ([B][N] of 0/1, or NULL).  A byte other than 0 / 1 is read as its low
// bit and flagged: returns qpd::ERR_MSG_BIT then, else 0.  Rows >= B are not touched.
inline int32_t encode_host(const Code &c, const uint8_t *msg, int64_t B, uint32_t mask, uint8_t *info, uint8_t *codeword) {
    const int N = c.N, K = c.K, A = c.A, nw = (N + 31) / 32, kw = (K + 31) / 32;
    std::vector<uint32_t> bw(kw + 2), xw(nw);
    int32_t flag = 0;
    for (int64_t f = 0; f < B; ++f) {
        const uint8_t *m = msg + f * A;
        std::fill(bw.begin(), bw.end(), 0u);
        uint32_t reg = 0, bad = 0;
        int j = 0;
        // 8 bytes at a time: bit i of the byte word's low bits -> bit j + i
        for (; j + 8 <= A; j += 8) {
            uint64_t v;
            std::memcpy(&v, m + j, 8);
            bad |= (v & 0xFEFEFEFEFEFEFEFEull) != 0;
            uint32_t b8 = 0;
            for (int i = 0; i < 8; ++i) b8 |= (uint32_t)((v >> (8 * i)) & 1u) << i;
            bw[j >> 5] |= b8 << (j & 31);
        }
        for (; j < A; ++j) {
            bad |= m[j] > 1;
            bw[j >> 5] |= (uint32_t)(m[j] & 1u) << (j & 31);
        }
        if (bad) flag |= qpd::ERR_MSG_BIT;
        if (c.crc_n) {  // CRC::encoding (utils.cpp:77-92): XOR of the set bits' contributions, then the mask
            for (int d = 0; d < kw; ++d)
                for (uint32_t mm = bw[d]; mm; mm &= mm - 1u) reg ^= c.crc_tab[32 * d + __builtin_ctz(mm)];
            reg ^= mask;
            for (int t = 0; t < K - A; ++t) {
                const uint32_t bit = (reg >> (c.crc_n - 1 - t)) & 1u;
                bw[(A + t) >> 5] |= bit << ((A + t) & 31);
            }
        }
        if (info)
            for (int t = 0; t < K; ++t) info[f * K + t] = (uint8_t)((bw[t >> 5] >> (t & 31)) & 1u);
        if (!codeword) continue;
        for (int w = 0; w < nw; ++w) {  // deposit, then the 5 in-word stages
            int s = c.info_pref[w];
            uint32_t u = 0;
            for (uint32_t mk = c.info_mask[w]; mk; mk &= mk - 1u, ++s)
                u |= ((bw[s >> 5] >> (s & 31)) & 1u) << __builtin_ctz(mk);
            u ^= (u >> 1) & 0x55555555u;
            u ^= (u >> 2) & 0x33333333u;
            u ^= (u >> 4) & 0x0F0F0F0Fu;
            u ^= (u >> 8) & 0x00FF00FFu;
            u ^= (u >> 16) & 0x0000FFFFu;
            xw[w] = u;
        }
        for (int sw = 1; sw < nw; sw <<= 1)  // word stages (m = 32 sw)
            for (int w = 0; w < nw; ++w)
                if (!(w & sw)) xw[w] ^= xw[w + sw];
        for (int i = 0; i < N; ++i) codeword[f * N + i] = (uint8_t)((xw[i >> 5] >> (i & 31)) & 1u);
    }
    return flag;
}

}  // namespace qpd_tx
