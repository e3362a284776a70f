"""LLR input of the LUT decoders, checked without a device: qpd_quantize_llr /
qpd_decode_llr / qpd_decode_llr_host are declared, exported and bound and the ABI
stays 7; the shared quantizer function (csrc/qpd_llr_quant.hpp -- the text the front
kernel and the host entry point call) agrees with a literal restatement of the driver's
loop in a stand-alone native program (address + undefined-behaviour sanitizers where
the compiler has them) and with codes.quantize_channel_scalar on the same vectors;
ChannelQuantizer validates; a float decoder's methods point to decode_batch."""
import ctypes
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import llr_vectors as V
from conftest import ROOT
from quantized_decoder_polar_codes_amd import _lib
from quantized_decoder_polar_codes_amd import codes as C

NAMES = {"qpd_quantize_llr": 7, "qpd_decode_llr": 7, "qpd_decode_llr_host": 6}
HEADER = os.path.join(ROOT, "include", "qpd.h")
CSRC = os.path.join(ROOT, "quantized_decoder_polar_codes_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")


@pytest.mark.parametrize("name", sorted(NAMES))
def test_declared_exported_and_bound(native_lib, name):
    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(rf"\bint {name}\(", txt)
    assert name in _lib.EXPORTED
    fn = getattr(native_lib, name)  # AttributeError: the library does not export it
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == NAMES[name]
    # (dec, ch, llr, llr_type, B, out [, stream])
    assert fn.argtypes[3] is ctypes.c_int32 and fn.argtypes[4] is ctypes.c_int64
    assert re.search(r"enum qpd_llr_type \{ QPD_LLR_F64 = 0, QPD_LLR_F32 = 1 \};", txt)
    assert (_lib.QPD_LLR_F64, _lib.QPD_LLR_F32) == (0, 1)


def test_abi_and_layouts_unchanged(native_lib):
    txt = open(HEADER).read()
    assert "#define QPD_ABI_VERSION 7" in txt and _lib.ABI_VERSION == 7 and native_lib.qpd_abi_version() == 7
    assert ctypes.sizeof(_lib.QpdInfo) == 96
    assert _lib.QPD_KC_COUNT == 4 and re.search(r"QPD_KC_COUNT = 4\b", txt)


def test_null_arguments_are_refused_without_a_device(native_lib):
    ch = _lib.QpdMcChannel()
    for name, n in NAMES.items():
        tail = (None,) * (n - 5)
        assert getattr(native_lib, name)(None, ctypes.byref(ch), None, 0, 4, *tail) == _lib.QPD_E_INVALID
        assert native_lib.qpd_last_error()


# ---------------------------------------------------------------------------------------------
# the shared function against the driver's loop
# ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def checker():
    """tests/native/llr_quant_check.cpp, host code: with the sanitizers where g++ links them and they start."""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "llr_quant_check")
    src = os.path.join(ROOT, "tests", "native", "llr_quant_check.cpp")
    base = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, src, "-o", exe + ".tmp"]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True)
    # without arguments the program exits with 2; a sanitizer runtime that cannot start here exits otherwise
    if san.returncode or subprocess.run([exe + ".tmp"], capture_output=True).returncode != 2:
        subprocess.run(base, check=True)
    os.replace(exe + ".tmp", exe)
    return exe


def _quantizers(native_lib):
    from quantized_decoder_polar_codes_amd import lutgen as LG

    return V.quantizers(LG)


@pytest.mark.parametrize("name", ["uniform", "mindistortion", "edges2", "edges257", "duplicates"])
def test_shared_function_is_the_drivers_loop(native_lib, checker, tmp_path, name):
    edges, lut, q = _quantizers(native_lib)[name]
    assert len(edges) == {"edges2": 2, "edges257": 257}.get(name, len(edges))
    x = np.concatenate([V.adversarial(edges, 2000, seed=11), [np.nan]])
    fin, fout = tmp_path / "in.txt", tmp_path / "out.txt"
    with open(fin, "w") as f:
        f.write(f"{q} {len(edges)}\n" + " ".join(float(e).hex() for e in edges) + "\n")
        f.write(" ".join(str(int(v)) for v in lut) + f"\n{x.size}\n")
        f.write("\n".join("%x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0] for v in x) + "\n")
    r = subprocess.run([checker, str(fin), str(fout)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert int(r.stdout) >= 2 * x.size  # each LLR also as the float32 the kernel would widen
    got = np.loadtxt(fout, dtype=np.int64)
    assert got[-1] == -1  # the NaN
    want = C.quantize_channel_scalar(x[:-1], edges, lut, q)
    assert np.array_equal(got[:-1], want)
    assert np.array_equal(C.quantize_channel(x[:-1], edges, lut, q), want)
    assert want.min() == 0 and want.max() == q - 1  # both saturations


# ---------------------------------------------------------------------------------------------
# the Python surface
# ---------------------------------------------------------------------------------------------

def test_channel_quantizer_validates_and_keeps_its_arrays(native_lib):
    import quantized_decoder_polar_codes_amd as Q
    from quantized_decoder_polar_codes_amd import lutgen as LG
    from quantized_decoder_polar_codes_amd import montecarlo as MC

    e, l = MC.uniform_channel_quantizer(16, 0.5)
    cq = Q.ChannelQuantizer(e, l, 16)
    assert (cq.ch.q, cq.ch.n_edges, cq.ch.sigma) == (16, 17, 0.0)
    assert cq.ch.edges == cq.edges.ctypes.data and cq.ch.lut == cq.lut.ctypes.data and cq.lut.dtype == np.int32
    assert Q.ChannelQuantizer(e, l).q == 16  # q from the lut
    _, _, ie, il = LG.channel_quantizer(0.8, 128, 16)
    md = Q.ChannelQuantizer(ie, il, 16)
    assert md.ch.n_edges == 129 and np.array_equal(md.lut, il)
    x = V.adversarial(ie, 500, seed=3)
    assert np.array_equal(md(x), C.quantize_channel(x, ie, il, 16))
    assert np.array_equal(Q.ChannelQuantizer.mindistortion(0.8).edges, md.edges)
    assert np.array_equal(Q.ChannelQuantizer.uniform(16, 0.5).edges, e)
    for bad in ((e[::-1], l, 16), (e, l[:-1], 16), (e, l, 15), (e[:1], l[:0], 2), (e, l + 0.5, 17), (e, -l, 16),
                (np.where(np.arange(17) == 3, np.nan, e), l, 16), (np.zeros(300), np.zeros(299, dtype=int), 2)):
        with pytest.raises(ValueError):
            Q.ChannelQuantizer(*bad)


def test_float_decoders_point_to_decode_batch(native_lib):
    import quantized_decoder_polar_codes_amd as Q

    N, K = 16, 8
    _, mb, fm, _ = C.construct_pw(N, K)
    flt = Q.SCDecoder(N, K, fm, 1 - fm, create=False)
    cq = Q.ChannelQuantizer.uniform()
    for call in (flt.decode_llr_batch, flt.quantize_llr):
        with pytest.raises(TypeError, match="decode_batch"):
            call(np.zeros((2, N)), cq)
