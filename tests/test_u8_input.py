"""uint8 channel symbols on the CPU side (qpd_decode_u8_host's small batches run the host engine's
``decode<uint8_t>``): the instantiation decodes the same bits and reports the same out-of-range symbols as
``decode<int32_t>``, in a g++ harness (tests/native/host_engine_u8_harness.cpp) fed the configuration the
Python classes hand to qpd_create; the same calls once more in a stand-alone program built with the address
and undefined-behaviour sanitizers (its own process, nothing loaded into Python); and the ABI the new entry
points arrive with.  The GPU side: tests/test_gpu_u8_input.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import code_masks as M
from conftest import ROOT

CSRC = os.path.join(ROOT, "quantized_decoder_polar_codes_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")
SRC = os.path.join(ROOT, "tests", "native", "host_engine_u8_harness.cpp")
DEPS = [SRC] + [os.path.join(CSRC, f) for f in ("qpd_host.hpp", "qpd_schedule.hpp", "qpd_types.hpp", "stl_sort.hpp")]
KINDS = ["SC-LUT", "SCL-LUT", "FastSC-LUT", "FastSCL-LUT"]
ERR_SYMBOL = 1  # qpd::ERR_SYMBOL (csrc/qpd_types.hpp)


def _stale(target):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in DEPS)


def _gxx(args, target):
    os.makedirs(BUILD, exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC] + args
                   + [SRC, "-o", target + ".tmp"], check=True)
    os.replace(target + ".tmp", target)


@pytest.fixture(scope="module")
def harness():
    so = os.path.join(BUILD, "host_engine_u8_harness.so")
    if _stale(so):
        _gxx(["-O3", "-fPIC", "-shared"], so)
    L = ctypes.CDLL(so)
    L.h8_decode.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int64] + [ctypes.c_void_p] * 2
    L.h8_decode.restype = ctypes.c_int
    return L


def _both(harness, dec, sym):
    """(flags of decode<int32_t>, flags of decode<uint8_t>, bits of each) on the same frames."""
    s32 = np.ascontiguousarray(sym, dtype=np.int32)
    s8 = np.ascontiguousarray(sym, dtype=np.uint8)
    assert (s8 == s32).all()
    o32 = np.full((len(sym), dec.out_bits), 7, dtype=np.uint8)
    o8 = np.full((len(sym), dec.out_bits), 9, dtype=np.uint8)
    rc = harness.h8_decode(ctypes.byref(dec._cfg), s32.ctypes.data, s8.ctypes.data, len(sym), o32.ctypes.data,
                           o8.ctypes.data)
    assert rc >= 0, rc
    return rc & 255, rc >> 8, o32, o8


def _decoder(kind, N, v, L):
    from quantized_decoder_polar_codes_amd import decoders as D
    from quantized_decoder_polar_codes_amd import lut as LU

    fm = M.named_mask(N, "random")
    assert not M.special_root(fm, kind)
    K = int((fm == 0).sum())
    p = LU.random_luts(N, v, seed=9 * N + v + L, distinct_mags=3)
    return D.from_packed(kind, p, K, fm, L=L, node_type=M.node_type_of(fm), create=False)


@pytest.mark.parametrize("L", [1, 4, 8])
@pytest.mark.parametrize("v", [2, 8, 16, 256])
@pytest.mark.parametrize("N", [8, 16, 128])
@pytest.mark.parametrize("kind", KINDS)
def test_host_engine_u8_equals_i32(kind, N, v, L, harness):
    """Same bits from both instantiations on tie-heavy tables; the symbol v is reported by both (v < 256), and
    255 is a symbol like any other at v = 256."""
    dec = _decoder(kind, N, v, L)
    sym = np.random.default_rng(N + v + L).integers(0, v, size=(12, N), dtype=np.int32)
    sym[0, :2] = (0, v - 1)  # both ends of the alphabet (255 at v = 256)
    f32, f8, o32, o8 = _both(harness, dec, sym)
    assert (f32, f8) == (0, 0)
    assert o32.max() <= 1 and (o32 == o8).all()
    if v < 256:
        for pos in (1, N // 2 + 1):
            bad = sym.copy()
            bad[5, pos] = v
            f32, f8, _, _ = _both(harness, dec, bad)
            assert (f32, f8) == (ERR_SYMBOL, ERR_SYMBOL), (pos, f32, f8)


def test_host_engine_u8_sanitized_program():
    """The harness as a stand-alone program under ASan + UBSan: every kind, N, v and L above once, checked
    by the program itself (exit status) -- run as a process of its own."""
    exe = os.path.join(BUILD, "host_engine_u8_san")
    if _stale(exe):
        # the runtimes linked into the program: it runs as it is wherever the suite runs
        _gxx(["-O1", "-g", "-DH8_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
              "-static-libasan", "-static-libubsan"], exe)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.search(r"host_engine_u8: 144 cases, 0 failed", r.stdout), r.stdout


def test_abi7_declares_the_u8_entry_points(native_lib):
    from quantized_decoder_polar_codes_amd import _lib

    with open(os.path.join(ROOT, "include", "qpd.h")) as f:
        txt = f.read()
    assert "#define QPD_ABI_VERSION 7" in txt and _lib.ABI_VERSION == 7 and native_lib.qpd_abi_version() == 7
    for name in ("qpd_decode_u8", "qpd_decode_u8_host"):
        assert name in _lib.EXPORTED and re.search(rf"\bint {name}\(", txt)
        assert getattr(native_lib, name).argtypes is not None
    # u8_staged took reserved0's place: the struct keeps its size and layout
    fields = [n for n, _ in _lib.QpdInfo._fields_]
    assert fields[-1] == "u8_staged" and "reserved0" not in fields
    assert ctypes.sizeof(_lib.QpdInfo) == 96
    assert re.search(r"int32_t u8_staged;", txt) and "reserved0" not in txt
