"""What tests/test_search_host.py and tests/test_gpu_search.py share: the plain-numpy references of
qpd_decode_search (include/qpd.h) -- a candidate's CRC syndrome from its K decisions, the set search
as R single-mask status decodes reduced by the rule of the header -- and the frames that make the
search matter: messages sent under three RNTIs through the host encoder at an SNR where some winners
sit at a rank above 0, noise-only frames, and a mask set that also holds two RNTIs nobody sent.
"""
from __future__ import annotations

import functools

import numpy as np

import status_cases as S
import status_ref


def mask_value(row):
    """M_i: the register value of a 0/1 mask row (qpd_status.hpp: bit l at register bit bits - 1 - l)."""
    v = 0
    for b in np.asarray(row).reshape(-1):
        v = (v << 1) | int(b)
    return v


def mask_rows(values, bits):
    """[R, bits] 0/1 rows of the integers `values`, most significant bit first."""
    return np.array([[(int(m) >> (bits - 1 - l)) & 1 for l in range(bits)] for m in values], dtype=np.uint8).reshape(len(values), bits)


def syndrome_ref(cand, A, chk, crc_n, crc_loc):
    """[B, L] uint32 from candidate bits [B, L, >= A + chk]: bit chk-1-j = CRC(info)[j] XOR tail bit j."""
    cand = np.asarray(cand)
    out = np.zeros(cand.shape[:2], dtype=np.uint32)
    for f in range(cand.shape[0]):
        for r in range(cand.shape[1]):
            cc = status_ref.crc_check_code(cand[f, r, :A], crc_n, crc_loc)[:chk]
            s = 0
            for j in range(chk):
                s |= int(cc[j] ^ cand[f, r, A + j]) << (chk - 1 - j)
            out[f, r] = s
    return out


def search_from_syndromes(syn, values, shift):
    """(hit_mask, hit_rank) by the header's pass rule on syndromes [B, L] and mask values M_i."""
    words = [int(v) >> shift for v in values]
    hit = np.full(len(syn), -1, dtype=np.int32)
    rank = np.zeros(len(syn), dtype=np.int32)
    for f, row in enumerate(syn):
        for r, s in enumerate(row):
            idx = [i for i, w in enumerate(words) if w == int(s)]
            if idx:
                hit[f], rank[f] = idx[0], r
                break
    return hit, rank


def stable_rank(pml, w):
    pw = pml[np.arange(len(w)), w][:, None]
    return ((pml < pw) | ((pml == pw) & (np.arange(pml.shape[1])[None] < w[:, None]))).sum(1).astype(np.int32)


def search_by_single_masks(walked, A, crc_n, crc_loc, rows):
    """The set search as R runs of status_ref.decode(..., mask=m_i) on the walked frames (status_ref.select
    is that function's output stage), reduced by the header's rule: the lowest rank any mask passes, then
    the lowest index; none: -1, rank 0, the unmasked run's best-metric path.  -> (out, hit, rank, metric)."""
    B = len(walked)
    assert len(rows) >= 1
    res = [None] * B  # per frame (rank, index, bits, metric) of the best passing run
    none = [None] * B  # ... and what a run that did not pass returned: the best-metric path
    for i, m in enumerate(rows):
        bits, pml, winner, passed = status_ref.select(walked, A, crc_n, crc_loc, m)
        rk = stable_rank(pml, winner)
        for f in range(B):
            if passed[f] and (res[f] is None or rk[f] < res[f][0]):
                res[f] = (int(rk[f]), i, bits[f], pml[f, winner[f]])
            if not passed[f]:
                assert rk[f] == 0
                none[f] = (0, -1, bits[f], pml[f, winner[f]])
    got = [res[f] or none[f] for f in range(B)]
    return (np.stack([g[2] for g in got]).astype(np.uint8), np.array([g[1] for g in got], dtype=np.int32),
            np.array([g[0] for g in got], dtype=np.int32), np.array([g[3] for g in got]))


# -- the frames that make the search matter --------------------------------------------------------------

# CA-SCL-LUT N = 128, A = 40, K = 64 (24 check bits = crc_n: a 16-bit RNTI is the syndrome itself), L = 8 on
# the min-sum tables.  Seed, SNR and frame counts were chosen on the CPU so that status_ref meets the
# conditions test_search_host.py asserts before it compares anything.
BLIND = S.Case("CA-SCL-LUT", 128, 64, 8, "minsum", A=40, crc_n=24)
RNTI_SENT = (0x1234, 0xBEEF, 0x0F0F)
RNTI_IDLE = (0x7777, 0xA5A5)
RNTI_SET = (RNTI_IDLE[0], RNTI_SENT[0], RNTI_SENT[1], RNTI_IDLE[1], RNTI_SENT[2])  # the search's set, 16 bits each
BLIND_SEED, BLIND_EBN0, BLIND_PER_MASK, BLIND_NOISE = 20261021, 0.5, 16, 12


@functools.lru_cache(maxsize=None)
def blind_frames(tx_exe, tmp_dir):
    """(symbols [B, N] int32, sent [B]: index into RNTI_SENT or -1 for noise only) -- the messages encoded
    under their RNTI by the host encoder (tests/native/tx_harness.cpp: qpd_encode_host's code), BPSK over
    numpy AWGN, the drivers' uniform 16-level quantizer; then the noise-only frames."""
    import pathlib

    import tx_cases as T

    c = BLIND
    fm, _, _ = S.code_of(c)
    rng = np.random.default_rng(BLIND_SEED)
    sigma = float(np.sqrt(1 / (2 * (c.K / c.N) * 10 ** (BLIND_EBN0 / 10))))
    ys, sent = [], []
    for i, rnti in enumerate(RNTI_SENT):
        msg = rng.integers(0, 2, size=(BLIND_PER_MASK, c.A), dtype=np.uint8)
        r = T.run_harness(tx_exe, pathlib.Path(tmp_dir), 0, T.KIND[c.kind], fm, msg, A=c.A, mask=mask_rows([rnti], 16)[0])
        assert r["rc"] == 0 and r["flag"] == 0, r["msg"]
        ys.append((1.0 - 2.0 * r["cw"]) + rng.normal(0, sigma, size=r["cw"].shape))
        sent += [i] * BLIND_PER_MASK
    ys.append(rng.normal(0, sigma, size=(BLIND_NOISE, c.N)))
    sent += [-1] * BLIND_NOISE
    llr = np.concatenate(ys) * 2 / sigma ** 2
    return np.clip(np.rint(llr / 0.5 + 7.5), 0, 15).astype(np.int32), np.array(sent)


@functools.lru_cache(maxsize=None)
def blind_reference(tx_exe, tmp_dir):
    """(x, sent, (out, hit, rank, metric), syndromes [B, L], cand_metric [B, L]) of the numpy restatement
    on the blind frames with RNTI_SET; computed once, not to be written to."""
    c = BLIND
    x, sent = blind_frames(tx_exe, tmp_dir)
    fm, _, _ = S.code_of(c)
    walked = [status_ref._decode_frame(S.tables_of(c), np.asarray(fm), c.L, y) for y in x]
    ref = search_by_single_masks(walked, c.A, c.crc_n, c.crc_loc, mask_rows(RNTI_SET, 16))
    order = [np.argsort(p, kind="stable") for _, p in walked]
    cand = np.stack([info[o] for (info, _), o in zip(walked, order)])
    cmet = np.stack([p[o] for (_, p), o in zip(walked, order)])
    return x, sent, ref, syndrome_ref(cand, c.A, c.K - c.A, c.crc_n, c.crc_loc), cmet


def check_blind_reference(sent, ref):
    """The conditions of the issue, on the reference's result alone."""
    out, hit, rank, metric = ref
    want = {RNTI_SET.index(r) for r in RNTI_SENT}
    assert want <= set(hit.tolist()), "every sent mask is hit at least once"
    assert not (set(hit.tolist()) - want - {-1}), "an idle RNTI was hit: choose another seed"
    assert (rank > 0).any(), "no frame has hit_rank > 0"
    assert (hit < 0).any(), "every frame is hit"
    assert len(hit) == len(sent) == 3 * BLIND_PER_MASK + BLIND_NOISE, "a frame is left out of the compare"
