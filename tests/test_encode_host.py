"""The transmit side (qpd_encode / qpd_encode_host / qpd_tx_frames, include/qpd.h) without a
GPU: the C-ABI's new symbols, and the host code of csrc/qpd_tx.hpp -- the argument rules and
the host encoder -- built with g++ into the stand-alone program tests/native/tx_harness.cpp
from the library's own sources, against codes.polar_encode and oracle.crc_encode; then the
encoder's words through the host engine and back.  The same on the kernels:
tests/test_gpu_encode.py and tests/test_gpu_tx_frames.py.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import tx_cases as T
from conftest import ROOT

NEW_SYMBOLS = ("qpd_encode", "qpd_encode_host", "qpd_tx_frames")


@pytest.fixture(scope="module")
def harness():
    return T.build_harness()


def test_abi_declares_exports_and_binds_tx():
    from quantized_decoder_polar_codes_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "qpd.h")).read()
    # additive: the ABI version and the structs are what they were
    assert re.search(r"#define QPD_ABI_VERSION 7\b", hdr) and _lib.ABI_VERSION == 7
    assert ctypes.sizeof(_lib.QpdInfo) == 96 and ctypes.sizeof(_lib.QpdStatusArgs) == 32
    assert ctypes.sizeof(_lib.QpdTxArgs) == 16 and "typedef struct qpd_tx_args" in hdr
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.EXPORTED
    assert (_lib.QPD_TX_SYM_I32, _lib.QPD_TX_SYM_U8, _lib.QPD_TX_LLR_F64) == (0, 1, 2)
    assert "PolarBDEnc.Encoder.PolarEnc" in hdr and "utils.cpp:77-92" in hdr  # what they replace
    so = os.path.join(ROOT, "quantized_decoder_polar_codes_amd", "libqpd.so")
    if os.path.exists(so):  # built: the symbols are exported (dlsym without initialising a device)
        L = ctypes.CDLL(so)
        for name in NEW_SYMBOLS:
            assert hasattr(L, name), name


# -- parity ------------------------------------------------------------------------------
def sc_grid():
    """(N, mask name) of the kinds without CRC: random and block masks and the edge masks."""
    out = [(4, "random"), (32, "random"), (64, "block2"), (128, "random"), (1024, "block5"), (4096, "random")]
    for N, name in ((32, "info0"), (64, "frozen_last"), (128, "K1_mid"), (64, "KN-1_mid"), (128, "alt10"), (32, "all_info"),
                    (1024, "alt10"), (4096, "KN-1_mid")):
        out.append((N, name))
    return out


@pytest.mark.parametrize("N,name", sc_grid(), ids=lambda v: str(v))
@pytest.mark.parametrize("B", (1, 67))
def test_host_encoder_matches_polar_encode(N, name, B, harness, tmp_path):
    fm = T.mask_for(N, name)
    K = int((fm == 0).sum())
    msg = np.random.default_rng(N + B).integers(0, 2, size=(B, K), dtype=np.uint8)
    want_info, want_cw = T.encode_ref(fm, msg)
    r = T.run_harness(harness, tmp_path, 0, T.KIND["SC"], fm, msg)
    assert r["rc"] == 0 and r["flag"] == 0
    assert (r["info"] == want_info).all() and (r["cw"] == want_cw).all()
    # each output alone: the same bytes
    r1 = T.run_harness(harness, tmp_path, 0, T.KIND["SC-LUT"], fm, msg, want_info=False)
    r2 = T.run_harness(harness, tmp_path, 0, T.KIND["SCL"], fm, msg, want_cw=False)
    assert r1["rc"] == 0 and r1["info"] is None and (r1["cw"] == want_cw).all()
    assert r2["rc"] == 0 and r2["cw"] is None and (r2["info"] == want_info).all()


def ca_grid():
    """(N, A, K - A, mask name): every A and every K - A of the issue's grid, sizes in turn."""
    out = []
    sizes = (128, 1024, 4096, 256)
    i = 0
    for A in (1, 31, 33, 64, 100):
        for t in (1, 8, 23, 24):
            N = sizes[i % len(sizes)]
            i += 1
            out.append((N, A, t, "random" if i % 3 else "block"))
    out += [(32, 1, 1, "random"), (64, 31, 8, "random"), (32, 7, 24, "random")]
    return out


def ca_mask(N, K, name):
    if name == "random":
        return T.mask_for(N, "random", K)
    # a block mask trimmed or topped up to K information positions (the blocks give no K to order)
    fm = T.M.block_mask(N, 5).copy()
    info, frozen = np.flatnonzero(fm == 0), np.flatnonzero(fm == 1)
    if info.size > K:
        fm[info[K:]] = 1
    else:
        fm[frozen[: K - info.size]] = 0
    return fm


MASKS = {0: np.zeros(0, np.uint8), 1: np.array([1], np.uint8),
         16: T.RNTI_MASK, 24: np.random.default_rng(24).integers(0, 2, size=24, dtype=np.uint8) | np.eye(24, dtype=np.uint8)[0]}


@pytest.mark.parametrize("N,A,t,name", ca_grid(), ids=lambda v: str(v))
def test_host_encoder_matches_crc_and_polar_encode(N, A, t, name, harness, tmp_path):
    K = A + t
    fm = ca_mask(N, K, name)
    assert int((fm == 0).sum()) == K
    for B in (1, 67):
        msg = np.random.default_rng(1000 * A + t + B).integers(0, 2, size=(B, A), dtype=np.uint8)
        plain = None
        for bits, mask in MASKS.items():
            want_info, want_cw = T.encode_ref(fm, msg, A=A, mask=mask)
            for kind in ("CA-SCL-LUT",) + (("CA-SCL",) if t == 24 else ()):
                r = T.run_harness(harness, tmp_path, 0, T.KIND[kind], fm, msg, A=A, mask=mask)
                assert r["rc"] == 0 and r["flag"] == 0, r["msg"]
                assert (r["info"] == want_info).all() and (r["cw"] == want_cw).all(), (bits, kind)
            if bits == 0:
                plain = want_cw
                r0 = T.run_harness(harness, tmp_path, 0, T.KIND["CA-FastSCL-LUT"], fm, msg, A=A)  # tx = NULL
                assert (r0["cw"] == plain).all()
            elif 24 - bits >= t or (bits == 24 and not mask[:t].any()):
                assert (want_cw == plain).all()
        # a mask whose set bits all lie beyond the K - A transmitted check bits changes nothing
        if t < 24:
            far = np.zeros(24, np.uint8)
            far[t:] = 1
            r = T.run_harness(harness, tmp_path, 0, T.KIND["CA-SCL-LUT"], fm, msg, A=A, mask=far)
            assert r["rc"] == 0 and (r["cw"] == plain).all()
            near = np.zeros(24, np.uint8)
            near[t - 1] = 1  # ... and the last transmitted one does
            r = T.run_harness(harness, tmp_path, 0, T.KIND["CA-SCL-LUT"], fm, msg, A=A, mask=near)
            assert r["rc"] == 0 and (r["cw"] != plain).any(1).all()


def test_other_crc_polynomials_and_lengths(harness, tmp_path):
    fm = T.mask_for(64, "random", 20 + 11)
    msg = np.random.default_rng(3).integers(0, 2, size=(67, 20), dtype=np.uint8)
    loc = (11, 10, 9, 5, 0)
    mask = np.array([1, 1, 0, 1], np.uint8)
    want_info, want_cw = T.encode_ref(fm, msg, A=20, crc_n=11, crc_loc=loc, mask=mask)
    r = T.run_harness(harness, tmp_path, 0, T.KIND["CA-SCL"], fm, msg, A=20, crc_n=11, crc_loc=loc, mask=mask)
    assert r["rc"] == 0 and (r["info"] == want_info).all() and (r["cw"] == want_cw).all()


# -- bad bytes, bounds --------------------------------------------------------------------
def test_bad_message_bytes_are_flagged_and_read_as_their_low_bit(harness, tmp_path):
    fm = T.mask_for(128, "random", 64)
    msg = np.random.default_rng(5).integers(0, 2, size=(9, 64), dtype=np.uint8)
    clean = T.run_harness(harness, tmp_path, 0, T.KIND["SC"], fm, msg)
    for bad, at in ((2, (4, 3)), (255, (4, 63)), (2, (0, 0)), (255, (8, 17))):
        m = msg.copy()
        m[at] = bad
        r = T.run_harness(harness, tmp_path, 0, T.KIND["SC"], fm, m)
        assert r["rc"] == 0 and r["flag"] == T.ERR_MSG_BIT  # rc 99 would be a write outside the rows
        want_info, want_cw = T.encode_ref(fm, m)  # (the reference masks the low bit)
        assert (r["info"] == want_info).all() and (r["cw"] == want_cw).all()
        others = np.arange(9) != at[0]
        assert (r["cw"][others] == clean["cw"][others]).all()  # the neighbouring frames are intact
    assert clean["flag"] == 0


# -- refusals ------------------------------------------------------------------------------
def test_encode_refusals_name_the_argument(harness, tmp_path):
    fm = T.mask_for(128, "random", 64)
    msg = np.zeros((2, 64), np.uint8)
    sc, ca = T.KIND["SC"], T.KIND["CA-SCL-LUT"]

    def run(kind=sc, **kw):
        r = T.run_harness(harness, tmp_path, 0, kind, fm, kw.pop("msg", msg), **kw)
        return r["rc"], r["msg"]

    assert run()[0] == 0
    rc, text = run(want_info=False, want_cw=False)
    assert rc == T.QPD_E_INVALID and "d_info" in text and "d_codeword" in text
    rc, text = run(mask=np.ones(1, np.uint8))
    assert rc == T.QPD_E_INVALID and "crc_mask" in text  # a mask on a kind without CRC
    rc, text = run(null_msg=True)
    assert rc == T.QPD_E_INVALID and "msg" in text
    rc, text = run(B=-1)
    assert rc == T.QPD_E_INVALID and "B" in text
    assert run(B=0, null_msg=True)[0] == 0  # an empty batch reads nothing
    rc, text = run(mask_bits=0, no_signal=1)
    assert rc == T.QPD_E_INVALID and "no_signal" in text
    cmsg = np.zeros((2, 40), np.uint8)
    assert run(ca, msg=cmsg, A=40, mask=np.ones(24, np.uint8))[0] == 0
    rc, text = run(ca, msg=cmsg, A=40, mask=np.ones(25, np.uint8))
    assert rc == T.QPD_E_INVALID and "crc_mask_bits" in text
    rc, text = run(ca, msg=cmsg, A=40, mask_bits=-2, mask=np.ones(2, np.uint8))
    assert rc == T.QPD_E_INVALID and "crc_mask_bits" in text
    rc, text = run(ca, msg=cmsg, A=40, mask=np.ones(4, np.uint8), null_mask=True)
    assert rc == T.QPD_E_INVALID and "crc_mask is NULL" in text
    rc, text = run(ca, msg=cmsg, A=40, mask=2 * np.ones(4, np.uint8))
    assert rc == T.QPD_E_INVALID and "0 or 1" in text
    # QPD_CASCL_FLOAT with A + crc_n < K: no check bits to fill the message with
    rc, text = run(T.KIND["CA-SCL"], msg=np.zeros((2, 30), np.uint8), A=30)
    assert rc == T.QPD_E_UNSUPPORTED and "K - A" in text
    assert run(99)[0] == T.QPD_E_INVALID  # no such kind


def test_tx_frames_refusals_name_the_argument(harness, tmp_path):
    fm = T.mask_for(128, "random", 64)
    msg = np.zeros((2, 64), np.uint8)
    I32, U8, F64 = 0, 1, 2

    def run(kind=T.KIND["SC"], **kw):
        r = T.run_harness(harness, tmp_path, 1, kind, fm, kw.pop("msg", msg), **kw)
        return r["rc"], r["msg"]

    for ty in (I32, U8, F64):
        assert run(out_type=ty)[0] == 0
    rc, text = run(out_type=3)
    assert rc == T.QPD_E_INVALID and "out_type" in text
    rc, text = run(has_ch=False)
    assert rc == T.QPD_E_INVALID and "ch" in text
    for ty in (I32, U8):
        rc, text = run(out_type=ty, has_rec=True)
        assert rc == T.QPD_E_INVALID and "rec" in text
    assert run(out_type=F64, has_rec=True)[0] == 0
    rc, text = run(out_type=U8, q=257)
    assert rc == T.QPD_E_INVALID and "q <= 256" in text
    assert run(out_type=I32, q=257)[0] == 0
    rc, text = run(null_frames=True)
    assert rc == T.QPD_E_INVALID and "d_frames" in text
    rc, text = run(null_msg=True)
    assert rc == T.QPD_E_INVALID and "d_msg" in text
    assert run(null_msg=True, mask_bits=0, no_signal=1)[0] == 0  # no_signal reads no message
    rc, text = run(frame0=-1)
    assert rc == T.QPD_E_INVALID and "frame0" in text
    rc, text = run(B=-1)
    assert rc == T.QPD_E_INVALID
    assert run(B=0, null_msg=True, null_frames=True)[0] == 0
    rc, text = run(out_type=F64, frames_offset=4)
    assert rc == T.QPD_E_INVALID and "alignment" in text
    rc, text = run(out_type=I32, frames_offset=2)
    assert rc == T.QPD_E_INVALID and "alignment" in text
    assert run(out_type=I32, frames_offset=4)[0] == 0 and run(out_type=U8, frames_offset=3)[0] == 0
    rc, text = run(mask=np.ones(3, np.uint8))
    assert rc == T.QPD_E_INVALID and "crc_mask" in text
    rc, text = run(T.KIND["CA-SCL"], msg=np.zeros((2, 30), np.uint8), A=30)
    assert rc == T.QPD_E_UNSUPPORTED


# -- round trips through the host engine -----------------------------------------------------
@pytest.mark.parametrize("kind,L", [("SC", 1), ("SCL", 4), ("CA-SCL", 4), ("FastSC", 1)])
def test_noiseless_round_trip_returns_the_message(kind, L, harness, tmp_path):
    from quantized_decoder_polar_codes_amd import codes as C

    N, K = 128, 64
    _, mb, fm, _ = C.construct_pw(N, K)
    A = K - 24 if kind == "CA-SCL" else K
    msg = np.random.default_rng(11).integers(0, 2, size=(40, A), dtype=np.uint8)
    nt = C.identify_nodes(N, mb).astype(np.int32) if kind == "FastSC" else None
    r = T.run_harness(harness, tmp_path, 2, T.KIND[kind], np.asarray(fm), msg, A=A if kind == "CA-SCL" else None, L=L,
                      mask_bits=0, node_type=nt)
    assert r["rc"] == 0, r["msg"]
    assert (r["bits"] == msg).all()
    if kind == "CA-SCL":
        assert (r["passed"] == 1).all()


def test_rnti_round_trip_passes_under_its_mask_only(harness, tmp_path):
    """The committed case of tests/tx_cases.py: 256 frames under a 16-bit mask."""
    fm, msg = T.rnti_case()
    args = dict(A=T.RNTI_A, L=T.RNTI_L, mask=T.RNTI_MASK)
    right = T.run_harness(harness, tmp_path, 2, T.KIND["CA-SCL"], fm, msg, dec_mask=T.RNTI_MASK, **args)
    assert right["rc"] == 0 and (right["passed"] == 1).all() and (right["bits"] == msg).all()
    wrong = T.run_harness(harness, tmp_path, 2, T.KIND["CA-SCL"], fm, msg, dec_mask=T.RNTI_OTHER, **args)
    assert wrong["rc"] == 0 and (wrong["passed"] == 0).all()
    none = T.run_harness(harness, tmp_path, 2, T.KIND["CA-SCL"], fm, msg, **args)  # and not without a mask
    assert none["rc"] == 0 and (none["passed"] == 0).all()
    # the oracle's CRC agrees on what was sent: the tail is crc ^ the placed mask
    import oracle

    enc = T.run_harness(harness, tmp_path, 0, T.KIND["CA-SCL"], fm, msg, A=T.RNTI_A, mask=T.RNTI_MASK)
    assert (enc["info"][:, T.RNTI_A:] == oracle.crc_encode(msg) ^ T.placed_mask(T.RNTI_MASK, 24)).all()
