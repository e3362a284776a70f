"""Decode status (qpd_decode_status / _host, include/qpd.h) without a GPU: the
C-ABI's new symbols, and the host engine's status run -- the host-engine branch of
qpd_decode_status_host, built with g++ into tests/native/status_harness.cpp from
the library's own sources (argument rules included), as tests/test_host_engine.py
reaches the engine:

* the reference's float CA-SCL with RNTI (CASCLWithRNTI.cpp:74-252), recorded in
  tests/golden/bd/bd_*.npz by tests/golden/make_bd_golden.py: bits, isPass and PM,
  PM as the same double;
* SCL-LUT / CA-SCL-LUT against tests/status_ref.py, itself first checked against
  the reference's own fixtures, with and without a 16-bit mask, metrics exact;
* the refusals.
The same on the kernels: tests/test_gpu_status.py.
"""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import status_ref
from conftest import GOLDEN_DIR, ROOT, golden_packed, load_golden

CSRC = os.path.join(ROOT, "quantized_decoder_polar_codes_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")
BD_FILES = sorted(glob.glob(os.path.join(GOLDEN_DIR, "bd", "bd_*.npz")))
MASK16 = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 1, 0, 1], dtype=np.uint8)
QPD_E_INVALID = -1


def build_status_harness():
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "status_harness.so")
    src = os.path.join(ROOT, "tests", "native", "status_harness.cpp")
    deps = [src, os.path.join(ROOT, "include", "qpd.h")] + [
        os.path.join(CSRC, f) for f in ("qpd_status.hpp", "qpd_host.hpp", "qpd_schedule.hpp", "qpd_types.hpp", "stl_sort.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.run(["g++", "-O3", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                        src, "-o", so + ".tmp"], check=True)
        os.replace(so + ".tmp", so)
    L = ctypes.CDLL(so)
    L.hs_decode_status.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p,
                                   ctypes.c_void_p]
    L.hs_decode_status.restype = ctypes.c_int
    return L


@pytest.fixture(scope="module")
def harness():
    return build_status_harness()


def host_status(harness, dec, x, mask=None, metric=True, crc_pass=True, mask_bits=None):
    """(rc, bits, metric, pass) of the host engine's status run on frames x."""
    from quantized_decoder_polar_codes_amd import _lib

    if dec._float_input:
        x, ty = np.ascontiguousarray(x, dtype=np.float64), _lib.QPD_IN_F64
    elif np.asarray(x).dtype == np.uint8:
        x, ty = np.ascontiguousarray(x), _lib.QPD_IN_U8
    else:
        x, ty = np.ascontiguousarray(x, dtype=np.int32), _lib.QPD_IN_I32
    B = len(x)
    out = np.zeros((B, dec.out_bits), dtype=np.uint8)
    m = np.full(B, -1.0)
    ok = np.full(B, 7, dtype=np.uint8)
    sa = _lib.QpdStatusArgs()
    if mask is not None:
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        sa.crc_mask, sa.crc_mask_bits = mask.ctypes.data, len(mask) if mask_bits is None else mask_bits
    if metric:
        sa.metric = m.ctypes.data
    if crc_pass:
        sa.crc_pass = ok.ctypes.data
    rc = harness.hs_decode_status(ctypes.byref(dec._cfg), x.ctypes.data, ty, B, out.ctypes.data, ctypes.byref(sa))
    return rc, out, m, ok


def bd_decoder(g, create=False, **kw):
    from quantized_decoder_polar_codes_amd.decoders import from_quant

    return from_quant("CA-SCL", int(g["N"]), int(g["K"]), g["frozen"], L=int(g["L"]), A=int(g["A"]),
                      crc_n=int(g["crc_n"]), crc_loc=g["crc_loc"], create=create, **kw)


def bd_groups(g):
    """The frames of a bd fixture by the RNTI their decode call took: (mask, frame indices)."""
    groups = {}
    for f in range(len(g["llr"])):
        groups.setdefault(tuple(g["rnti"][f, : g["rnti_len"][f]].tolist()), []).append(f)
    return [(np.array(k, dtype=np.uint8), np.array(v)) for k, v in groups.items()]


def test_abi_declares_exports_and_binds_status():
    from quantized_decoder_polar_codes_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "qpd.h")).read()
    assert re.search(r"#define QPD_ABI_VERSION 7\b", hdr) and _lib.ABI_VERSION == 7
    assert ctypes.sizeof(_lib.QpdInfo) == 96
    for name in ("qpd_decode_status", "qpd_decode_status_host"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.EXPORTED
    assert "typedef struct qpd_status_args" in hdr
    assert ctypes.sizeof(_lib.QpdStatusArgs) == 32
    assert (_lib.QPD_IN_I32, _lib.QPD_IN_U8, _lib.QPD_IN_F64) == (0, 1, 2)
    so = os.path.join(ROOT, "quantized_decoder_polar_codes_amd", "libqpd.so")
    if os.path.exists(so):  # built: the symbols are exported (dlsym without initialising a device)
        L = ctypes.CDLL(so)
        for name in ("qpd_decode_status", "qpd_decode_status_host"):
            assert hasattr(L, name), name


def test_bd_fixtures_are_informative():
    assert len(BD_FILES) == 4
    for path in BD_FILES:
        g = load_golden(path)
        assert g["is_pass"].sum() >= 8 and (~g["is_pass"]).sum() >= 8
        assert g["frozen"][-1] == 0  # PM is then the winner's own metric
        assert sorted(set(g["rnti_len"].tolist())) == [0, 16]
    # conftest.golden_files() must not hand them to the plain decoders' tests
    from conftest import golden_files

    assert not [p for p in golden_files() + golden_files("float_*.npz") if os.path.basename(p).startswith("bd_")]


@pytest.mark.parametrize("path", BD_FILES, ids=lambda p: os.path.basename(p)[:-4])
def test_host_engine_reproduces_reference_bd(path, harness):
    g = load_golden(path)
    dec = bd_decoder(g)
    for mask, idx in bd_groups(g):
        rc, bits, m, ok = host_status(harness, dec, g["llr"][idx], mask=mask if len(mask) else None)
        assert rc == 0
        assert (bits == g["bits"][idx]).all()
        assert (ok == g["is_pass"][idx]).all()
        assert (m == g["pm"][idx]).all(), np.abs(m - g["pm"][idx]).max()  # the same doubles


LUT_CASES = [("scllut_n128_k64_l8_random", None), ("ca_scllut_n128_a40_l8_minsum", 40)]


@pytest.fixture(scope="module")
def lut_refs():
    """status_ref on the reference's fixtures, once: {(name, masked): (bits, pml, winner, passed)}."""
    refs = {}
    for name, A in LUT_CASES:
        g = load_golden(os.path.join(GOLDEN_DIR, name + ".npz"))
        p = golden_packed(g)
        for masked in ((False, True) if A else (False,)):
            refs[name, masked] = status_ref.decode(p, g["frozen"], int(g["L"]), g["symbols"], A=A,
                                                   mask=MASK16 if masked else None)
    return refs


@pytest.mark.parametrize("name,A", LUT_CASES)
def test_status_ref_reproduces_reference_bits(name, A, lut_refs):
    g = load_golden(os.path.join(GOLDEN_DIR, name + ".npz"))
    assert (lut_refs[name, False][0] == g["expected"]).all()


def lut_decoder(g, A, create=False, **kw):
    from quantized_decoder_polar_codes_amd import decoders as D

    kind = "CA-SCL-LUT" if A else "SCL-LUT"
    return D.from_packed(kind, golden_packed(g), int(g["K"]), g["frozen"], L=int(g["L"]), create=create,
                         **({"A": A} if A else {}), **kw)


# (a mask needs a CRC: SCL-LUT with a mask is one of test_refusals')
@pytest.mark.parametrize("name,A,masked", [LUT_CASES[0] + (False,), LUT_CASES[1] + (False,), LUT_CASES[1] + (True,)])
def test_host_engine_status_matches_restatement(name, A, masked, harness, lut_refs):
    g = load_golden(os.path.join(GOLDEN_DIR, name + ".npz"))
    bits, pml, win, passed = lut_refs[name, masked]
    rc, got, m, ok = host_status(harness, lut_decoder(g, A), g["symbols"], mask=MASK16 if masked else None,
                                 crc_pass=bool(A))
    assert rc == 0
    assert (got == bits).all()
    assert (m == pml[np.arange(len(win)), win]).all()
    if A:
        assert (ok == passed).all()
        if masked:  # the mask changes the verdicts: most frames pass without it, few with it
            assert passed.sum() < lut_refs[name, False][3].sum()
    # uint8 symbols: the same status
    rc8, got8, m8, ok8 = host_status(harness, lut_decoder(g, A), g["symbols"].astype(np.uint8),
                                     mask=MASK16 if masked else None, crc_pass=bool(A))
    assert rc8 == 0 and (got8 == got).all() and (m8 == m).all() and (not A or (ok8 == ok).all())


def test_outputs_are_optional_and_independent(harness):
    name, A = LUT_CASES[1]
    g = load_golden(os.path.join(GOLDEN_DIR, name + ".npz"))
    dec = lut_decoder(g, A)
    _, bits, m, ok = host_status(harness, dec, g["symbols"])
    _, b1, m1, ok1 = host_status(harness, dec, g["symbols"], crc_pass=False)
    _, b2, m2, ok2 = host_status(harness, dec, g["symbols"], metric=False)
    assert (b1 == bits).all() and (m1 == m).all() and (ok1 == 7).all()
    assert (b2 == bits).all() and (m2 == -1.0).all() and (ok2 == ok).all()
    assert (bits == g["expected"]).all()


def test_refusals(harness):
    from quantized_decoder_polar_codes_amd import decoders as D
    from quantized_decoder_polar_codes_amd import _lib

    g = load_golden(os.path.join(GOLDEN_DIR, LUT_CASES[0][0] + ".npz"))
    scl = lut_decoder(g, None)
    sym = g["symbols"][:2]
    assert host_status(harness, scl, sym, crc_pass=False)[0] == 0
    assert host_status(harness, scl, sym, crc_pass=True)[0] == QPD_E_INVALID  # crc_pass without a CRC
    assert host_status(harness, scl, sym, mask=MASK16, crc_pass=False)[0] == QPD_E_INVALID  # a mask without a CRC
    sc = D.from_packed("SC-LUT", golden_packed(g), int(g["K"]), g["frozen"], create=False)
    assert host_status(harness, sc, sym, crc_pass=False)[0] == QPD_E_INVALID  # SC has no metric
    assert host_status(harness, sc, sym, metric=False)[0] == QPD_E_INVALID
    assert host_status(harness, sc, sym, metric=False, crc_pass=False)[0] == 0  # nothing asked: the plain decode
    gc = load_golden(os.path.join(GOLDEN_DIR, LUT_CASES[1][0] + ".npz"))
    ca = lut_decoder(gc, 40)
    assert host_status(harness, ca, gc["symbols"][:2], mask=np.ones(24, dtype=np.uint8))[0] == 0
    assert host_status(harness, ca, gc["symbols"][:2], mask=np.ones(25, dtype=np.uint8))[0] == QPD_E_INVALID
    assert host_status(harness, ca, gc["symbols"][:2], mask=MASK16, mask_bits=-1)[0] == QPD_E_INVALID
    assert host_status(harness, ca, gc["symbols"][:2], mask=2 * MASK16)[0] == QPD_E_INVALID  # entries are 0 / 1
    # the input type must be the decoder's
    x = np.zeros((1, int(gc["N"])))
    out = np.zeros((1, 40), dtype=np.uint8)
    sa = _lib.QpdStatusArgs()
    assert harness.hs_decode_status(ctypes.byref(ca._cfg), x.ctypes.data, _lib.QPD_IN_F64, 1, out.ctypes.data,
                                    ctypes.byref(sa)) == QPD_E_INVALID


def test_polarbd_shim_rejects_a_list_larger_than_the_code():
    from PolarBD.PolarBD.CASCLWithRNTI import CASCLDecoder

    frozen = np.ones(8, dtype=np.int32)
    frozen[[6, 7]] = 0
    with pytest.raises(ValueError, match="2\\^K < L"):
        CASCLDecoder(8, 2, 1, 8, frozen, 1 - frozen, 1, [1, 0])
