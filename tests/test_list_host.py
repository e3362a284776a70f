"""List output (qpd_decode_list / _host, include/qpd.h) without a GPU: the C-ABI's new
symbols, and the host engine's list run -- the host-engine branch of
qpd_decode_list_host, built with g++ into tests/native/list_harness.cpp from the
library's own sources (argument rules included), as tests/test_status_host.py reaches
the status run:

* SCL-LUT / CA-SCL-LUT against tests/list_ref.py (all paths of tests/status_ref.py, which
  test_status_host.py checks against the reference's fixtures), exactly: bits, metrics as
  the same doubles, pass flags and the chosen candidate, with and without a 16-bit mask;
* every list kind the host engine decodes, L = 12 and 16 included, against the CPU oracle's
  status (every path's metric, the winner, the bits);
* the reference's float CA-SCL with RNTI (tests/golden/bd/bd_*.npz);
* the refusals.
The same on the kernels: tests/test_gpu_list.py.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import list_ref
import status_cases as S
from conftest import ROOT, load_golden
from test_status_host import BD_FILES, MASK16, bd_decoder, bd_groups

CSRC = os.path.join(ROOT, "quantized_decoder_polar_codes_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")
QPD_E_INVALID, QPD_E_UNSUPPORTED = -1, -2


def build_list_harness():
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "list_harness.so")
    src = os.path.join(ROOT, "tests", "native", "list_harness.cpp")
    deps = [src, os.path.join(ROOT, "include", "qpd.h")] + [
        os.path.join(CSRC, f) for f in ("qpd_list.hpp", "qpd_status.hpp", "qpd_host.hpp", "qpd_schedule.hpp",
                                        "qpd_types.hpp", "stl_sort.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.run(["g++", "-O3", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                        src, "-o", so + ".tmp"], check=True)
        os.replace(so + ".tmp", so)
    L = ctypes.CDLL(so)
    L.hl_decode_list.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p,
                                 ctypes.c_void_p]
    L.hl_decode_list.restype = ctypes.c_int
    return L


@pytest.fixture(scope="module")
def harness():
    return build_list_harness()


def host_list(harness, dec, x, mask=None, bits=True, metric=True, crc_pass=True, chosen=True, out=True, mask_bits=None):
    """(rc, bits [B, L, K], metric, pass, chosen, out) of the host engine's list run on frames x; what is
    not asked for keeps its canary (bits 0xEE, metric -7, pass 0x55, chosen -3, out 0xDD)."""
    from quantized_decoder_polar_codes_amd import _lib

    if dec._float_input:
        x, ty = np.ascontiguousarray(x, dtype=np.float64), _lib.QPD_IN_F64
    elif np.asarray(x).dtype == np.uint8:
        x, ty = np.ascontiguousarray(x), _lib.QPD_IN_U8
    else:
        x, ty = np.ascontiguousarray(x, dtype=np.int32), _lib.QPD_IN_I32
    B, L, K = len(x), int(dec.L), int(dec.K)
    o = np.full((B, dec.out_bits), 0xDD, dtype=np.uint8)
    b = np.full((B, L, K), 0xEE, dtype=np.uint8)
    m = np.full((B, L), -7.0)
    ok = np.full((B, L), 0x55, dtype=np.uint8)
    ch = np.full(B, -3, dtype=np.int32)
    la = _lib.QpdListArgs()
    if mask is not None:
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        la.crc_mask, la.crc_mask_bits = mask.ctypes.data, len(mask) if mask_bits is None else mask_bits
    if bits:
        la.cand_bits = b.ctypes.data
    if metric:
        la.cand_metric = m.ctypes.data
    if crc_pass:
        la.cand_pass = ok.ctypes.data
    if chosen:
        la.chosen = ch.ctypes.data
    rc = harness.hl_decode_list(ctypes.byref(dec._cfg), x.ctypes.data, ty, B, o.ctypes.data if out else None,
                                ctypes.byref(la))
    return rc, b, m, ok, ch, o


def host_decoder(c):
    from quantized_decoder_polar_codes_amd import decoders as D

    fm, nt, _ = S.code_of(c)
    kw = dict(A=c.A, crc_n=c.crc_n, crc_loc=c.crc_loc) if c.A else {}
    if c.is_float:
        return D.from_quant(c.kind, c.N, c.K, fm, L=c.L, node_type=nt, quant=S.quant_of(c), create=False, **kw)
    return D.from_packed(c.kind, S.tables_of(c), c.K, fm, L=c.L, node_type=nt, create=False, **kw)


def test_abi_declares_exports_and_binds_list():
    from quantized_decoder_polar_codes_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "qpd.h")).read()
    assert re.search(r"#define QPD_ABI_VERSION 7\b", hdr) and _lib.ABI_VERSION == 7
    assert ctypes.sizeof(_lib.QpdInfo) == 96 and ctypes.sizeof(_lib.QpdStatusArgs) == 32
    for name in ("qpd_decode_list", "qpd_decode_list_host"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.EXPORTED
    assert "typedef struct qpd_list_args" in hdr
    assert ctypes.sizeof(_lib.QpdListArgs) == 48
    assert "L > 16" in hdr and "introsort" in hdr  # the header says why larger lists are refused
    so = os.path.join(ROOT, "quantized_decoder_polar_codes_amd", "libqpd.so")
    if os.path.exists(so):  # built: the symbols are exported (dlsym without initialising a device)
        L = ctypes.CDLL(so)
        for name in ("qpd_decode_list", "qpd_decode_list_host"):
            assert hasattr(L, name), name


# -- SCL-LUT / CA-SCL-LUT against the restatement, exactly --------------------------------------------------

def small_case(N, L, ca):
    """N = 16: K = 14 (A = 4: check bits 0..9, of which a 16-bit mask meets 8 and 9); N = 64: K = 32 (A = 16)."""
    K = 14 if N == 16 else 32
    if ca:
        return S.Case("CA-SCL-LUT", N, K, L, "minsum", A=4 if N == 16 else 16, crc_n=24, ebn0=1.0, B=24)
    return S.Case("SCL-LUT", N, K, L, "random", B=24)


@pytest.mark.parametrize("ca", [False, True], ids=["scl", "ca"])
@pytest.mark.parametrize("L", [2, 4, 8])
@pytest.mark.parametrize("N", [16, 64])
def test_host_list_matches_restatement(N, L, ca, harness):
    c = small_case(N, L, ca)
    fm, _, _ = S.code_of(c)
    x = S.inputs_of(c)
    dec = host_decoder(c)
    for mask in ((None, MASK16) if ca else (None,)):
        wb, wm, wp, wc = list_ref.decode(S.tables_of(c), fm, L, x, A=c.A or None, mask=mask)
        rc, b, m, ok, ch, out = host_list(harness, dec, x, mask=mask, crc_pass=ca)
        assert rc == 0
        assert (b == wb).all()
        assert (m == wm).all()  # the same doubles
        assert (ch == wc).all()
        assert (out == wb[np.arange(len(x)), wc][:, : dec.out_bits]).all()
        if ca:
            assert (ok == wp).all()
        else:
            assert (ok == 0x55).all()
    # uint8 symbols: the same list
    rc8, b8, m8, ok8, ch8, out8 = host_list(harness, dec, x.astype(np.uint8), mask=mask, crc_pass=ca)
    assert rc8 == 0 and (b8 == b).all() and (m8 == m).all() and (ok8 == ok).all() and (ch8 == ch).all() and (out8 == out).all()


# -- every list kind of the host engine against the oracle's status ----------------------------------------

ORACLE_CASES = [
    S.Case("SCL-LUT", 64, 32, 12, "random", B=32),
    S.Case("SCL-LUT", 64, 32, 16, "minsum", B=32),
    S.Case("FastSCL-LUT", 128, 64, 8, "minsum", B=32),
    S.Case("FastSCL-LUT", 128, 64, 16, "random", B=32),
    S.Case("CA-SCL-LUT", 64, 40, 12, "minsum", A=16, crc_n=24, ebn0=1.0, B=32),
    S.Case("CA-SCL-LUT", 64, 40, 16, "minsum", A=16, crc_n=24, ebn0=1.0, B=32),
    S.Case("CA-FastSCL-LUT", 128, 64, 8, "minsum", A=40, crc_n=24, ebn0=1.0, B=32),
    S.Case("CA-FastSCL-LUT", 128, 64, 12, "minsum", A=40, crc_n=24, ebn0=1.0, B=32),
    S.Case("SCL", 64, 32, 4, "ties", B=32),
    S.Case("SCL", 64, 32, 16, "ties", B=32),
    S.Case("FastSCL", 128, 64, 12, "ties", B=32),
    S.Case("CA-SCL", 64, 32, 8, "ties", A=21, crc_n=11, ebn0=1.0, B=32),
    S.Case("CA-SCL", 64, 32, 16, "awgn", A=21, crc_n=11, ebn0=1.0, B=32),
]


def stable_rank(pml, w):
    rows = np.arange(len(w))
    pw = pml[rows, w][:, None]
    return ((pml < pw) | ((pml == pw) & (np.arange(pml.shape[1])[None] < w[:, None]))).sum(1)


def check_against_oracle(c, ref, b, m, ok, ch, out):
    """The list outputs of one call against the oracle's status (bits, pml, winner, passed)."""
    bits, pml, winner, passed = ref
    rows = np.arange(len(winner))
    assert (m == np.sort(pml, axis=1, kind="stable")).all(), "metrics: the oracle's, sorted"
    assert (ch == stable_rank(pml, winner)).all(), "chosen: the oracle winner's stable rank"
    assert (b[rows, ch][:, : bits.shape[1]] == bits).all(), "the chosen candidate's bits"
    assert (out == bits).all()
    if c.A:
        assert (ok.any(1) == passed).all()
        first = np.where(ok.any(1), ok.argmax(1), 0)
        assert (ch == first).all(), "chosen: the first passing candidate, else 0"
    else:
        assert (ch == 0).all()


@pytest.mark.parametrize("c", ORACLE_CASES, ids=lambda c: c.id)
def test_host_list_matches_oracle_status(c, harness, oracle_mod):
    assert not S.special_root(c)
    x, ref = S.reference(c)
    dec = host_decoder(c)
    for mb, want in ref.items():
        rc, b, m, ok, ch, out = host_list(harness, dec, x, mask=S.crc_mask(mb) if mb else None, crc_pass=bool(c.A))
        assert rc == 0, c.id
        check_against_oracle(c, want, b, m, ok.astype(bool), ch, out)


# -- the reference's CASCLWithRNTI ---------------------------------------------------------------------------

@pytest.mark.parametrize("path", BD_FILES, ids=lambda p: os.path.basename(p)[:-4])
def test_host_list_reproduces_reference_bd(path, harness):
    """The fourth fixture is recorded at L = 32, which qpd_decode_list refuses (the argsort is the
    unstable introsort above 16 paths): there the refusal is what is checked."""
    g = load_golden(path)
    dec = bd_decoder(g)
    for mask, idx in bd_groups(g):
        rc, b, m, ok, ch, out = host_list(harness, dec, g["llr"][idx], mask=mask if len(mask) else None)
        if int(g["L"]) > 16:
            assert rc == QPD_E_UNSUPPORTED and (b == 0xEE).all() and (out == 0xDD).all()
            continue
        assert rc == 0
        assert (out == g["bits"][idx]).all()
        assert (m[np.arange(len(idx)), ch] == g["pm"][idx]).all()  # the same doubles
        assert (ok.astype(bool).any(1) == g["is_pass"][idx]).all()
        assert (np.diff(m, axis=1) >= 0).all()


# -- optional outputs, refusals --------------------------------------------------------------------------------

def test_outputs_are_optional_and_independent(harness):
    c = small_case(64, 8, True)
    x, dec = S.inputs_of(c), host_decoder(c)
    _, b, m, ok, ch, out = host_list(harness, dec, x)
    rc, b1, m1, ok1, ch1, out1 = host_list(harness, dec, x, metric=False, crc_pass=False, chosen=False, out=False)
    assert rc == 0 and (b1 == b).all()
    assert (m1 == -7.0).all() and (ok1 == 0x55).all() and (ch1 == -3).all() and (out1 == 0xDD).all()
    rc, b2, m2, ok2, ch2, out2 = host_list(harness, dec, x, metric=False)
    assert rc == 0 and (b2 == b).all() and (ok2 == ok).all() and (ch2 == ch).all() and (out2 == out).all()


def test_refusals(harness):
    from quantized_decoder_polar_codes_amd import decoders as D
    from quantized_decoder_polar_codes_amd import _lib

    c = small_case(64, 4, False)
    fm, nt, _ = S.code_of(c)
    x = S.inputs_of(c)[:2]
    scl = host_decoder(c)
    assert host_list(harness, scl, x, crc_pass=False)[0] == 0
    assert host_list(harness, scl, x, crc_pass=True)[0] == QPD_E_INVALID  # cand_pass without a CRC
    assert host_list(harness, scl, x, mask=MASK16, crc_pass=False)[0] == QPD_E_INVALID  # a mask without a CRC
    assert host_list(harness, scl, x, bits=False, crc_pass=False)[0] == QPD_E_INVALID  # cand_bits is required
    for kind in ("SC-LUT", "FastSC-LUT"):
        sc = D.from_packed(kind, S.tables_of(c), c.K, fm, node_type=nt, create=False)
        assert host_list(harness, sc, x, crc_pass=False)[0] == QPD_E_INVALID  # no list
    one = host_decoder(c._replace(L=1))
    assert host_list(harness, one, x, crc_pass=False)[0] == QPD_E_UNSUPPORTED
    assert host_list(harness, one, x, mask=MASK16, crc_pass=False)[0] == QPD_E_INVALID  # (the mask rule first)
    wide = host_decoder(c._replace(L=32))
    assert host_list(harness, wide, x, crc_pass=False)[0] == QPD_E_UNSUPPORTED  # L > 16: introsort order
    assert host_list(harness, host_decoder(c._replace(L=16)), x, crc_pass=False)[0] == 0
    cc = small_case(64, 4, True)
    ca, xc = host_decoder(cc), S.inputs_of(cc)[:2]
    assert host_list(harness, ca, xc, mask=np.ones(24, dtype=np.uint8))[0] == 0
    assert host_list(harness, ca, xc, mask=np.ones(25, dtype=np.uint8))[0] == QPD_E_INVALID
    assert host_list(harness, ca, xc, mask=MASK16, mask_bits=-1)[0] == QPD_E_INVALID
    assert host_list(harness, ca, xc, mask=2 * MASK16)[0] == QPD_E_INVALID  # entries are 0 / 1
    # no argument struct; an input type that is not the decoder's
    out = np.zeros((2, ca.out_bits), dtype=np.uint8)
    xi = np.ascontiguousarray(xc, dtype=np.int32)
    assert harness.hl_decode_list(ctypes.byref(ca._cfg), xi.ctypes.data, _lib.QPD_IN_I32, 2, out.ctypes.data, None) == QPD_E_INVALID
    la = _lib.QpdListArgs()
    b = np.zeros((2, 4, cc.K), dtype=np.uint8)
    la.cand_bits = b.ctypes.data
    xf = np.zeros((2, cc.N))
    assert harness.hl_decode_list(ctypes.byref(ca._cfg), xf.ctypes.data, _lib.QPD_IN_F64, 2, out.ctypes.data,
                                  ctypes.byref(la)) == QPD_E_INVALID
