"""The float64-LLR Monte-Carlo entry points' surface, checked without a device:
qpd_mc_llr / qpd_mc_decode_f64 are declared, exported and bound; a null handle is
refused before any device call; and the chunk rule the header documents is the
one the library (csrc/qpd_chunk.hpp) and the Python helper compute."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT
from quantized_decoder_polar_codes_amd import _lib
from quantized_decoder_polar_codes_amd import montecarlo as MC

NAMES = ("qpd_mc_llr", "qpd_mc_decode_f64")
HEADER = os.path.join(ROOT, "include", "qpd.h")
CSRC = os.path.join(ROOT, "quantized_decoder_polar_codes_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")


@pytest.mark.parametrize("name", NAMES)
def test_declared_exported_and_bound(native_lib, name):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(rf"\bint {name}\(", txt)
    assert name in _lib.EXPORTED
    fn = getattr(native_lib, name)  # AttributeError: the library does not export it
    assert fn.argtypes is not None and fn.restype is ctypes.c_int
    # (dec, ch, rec, seed, frame0, B, d_msg, d_llr | d_out [, d_counts], stream)
    assert len(fn.argtypes) == (9 if name == "qpd_mc_llr" else 10)
    assert fn.argtypes[3] is ctypes.c_uint64 and fn.argtypes[4] is ctypes.c_int64 and fn.argtypes[5] is ctypes.c_int64


def test_abi_version_unchanged(native_lib):
    assert "#define QPD_ABI_VERSION 7" in open(HEADER).read() and native_lib.qpd_abi_version() == 7


def test_null_handle_is_refused_without_a_device(native_lib):
    ch = _lib.QpdMcChannel()
    ch.sigma = 1.0
    rc = native_lib.qpd_mc_llr(None, ctypes.byref(ch), None, ctypes.c_uint64(1), 0, 4, None, None, None)
    assert rc == _lib.QPD_E_INVALID and native_lib.qpd_last_error()
    rc = native_lib.qpd_mc_decode_f64(None, ctypes.byref(ch), None, ctypes.c_uint64(1), 0, 4, None, None, None, None)
    assert rc == _lib.QPD_E_INVALID and native_lib.qpd_last_error()


def test_chunk_rule_is_the_documented_one():
    """max(1, 2^28 / (8 N)) frames: the header's sentence, the library's helper
    (compiled here, host code without HIP) and montecarlo.llr_chunk_frames."""
    txt = " ".join(open(HEADER).read().split())
    assert "frames per chunk = max(1, 2^28 / (8 N))" in txt
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "mc_llr_chunk_check")
    src = os.path.join(ROOT, "tests", "native", "mc_llr_chunk_check.cpp")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I", CSRC, src, "-o", exe + ".tmp"], check=True)
    os.replace(exe + ".tmp", exe)
    Ns = [2, 1024, 65536]
    out = subprocess.run([exe] + [str(n) for n in Ns], capture_output=True, text=True, check=True).stdout.split()
    want = [max(1, 2 ** 28 // (8 * n)) for n in Ns]
    assert [int(x) for x in out] == want == [MC.llr_chunk_frames(n) for n in Ns]
    assert want == [1 << 24, 32768, 512]
