"""The blind-detection metric (qpd_dmetric / qpd_dmetric_host, include/qpd.h) without a
GPU: the C-ABI's new symbols, and the host-engine branch of qpd_dmetric_host -- the
argument rules of csrc/qpd_dmetric.hpp and the host engine's metric run, built with g++
into the stand-alone program tests/native/dmetric_harness.cpp from the library's own
sources -- against

* the reference's own doubles, DMetricCalculator::calculate (DMetric.cpp:24-177) recorded
  in tests/golden/dmetric/dm_*.npz by tests/golden/make_dmetric_golden.py;
* tests/dmetric_ref.py (itself checked against those fixtures, tests/test_dmetric_ref.py)
  on block and edge masks of tests/code_masks.py at N = 8, 16, 64, 256.
Every metric is compared as the same double, every frame counts.  The drop-in class
PolarBD.PolarBD.DMetricCalculator needs a decoder, hence a device: its case is marked gpu
and runs on the host engine.  The same on the kernel: tests/test_gpu_dmetric.py.
"""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import code_masks as M
import dmetric_ref
from conftest import GOLDEN_DIR, ROOT, assert_engine, load_golden

CSRC = os.path.join(ROOT, "quantized_decoder_polar_codes_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")
DM_FILES = sorted(glob.glob(os.path.join(GOLDEN_DIR, "dmetric", "dm_*.npz")))
QPD_E_INVALID = -1
QPD_FASTSC_FLOAT, QPD_SCL_FLOAT, QPD_SC_LUT, QPD_FASTSC_LUT = 9, 7, 1, 3
NEW_SYMBOLS = ("qpd_dmetric", "qpd_dmetric_host")


@pytest.fixture(scope="module")
def harness():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "dmetric_harness")
    src = os.path.join(ROOT, "tests", "native", "dmetric_harness.cpp")
    deps = [src, os.path.join(ROOT, "include", "qpd.h")] + [
        os.path.join(CSRC, f) for f in ("qpd_dmetric.hpp", "qpd_host.hpp", "qpd_schedule.hpp", "qpd_types.hpp", "stl_sort.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-O3", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC, src, "-o", exe + ".tmp"],
                       check=True)
        os.replace(exe + ".tmp", exe)
    return exe


def host_dmetric(exe, tmp_path, kind, N, K, frozen, node_type, llr, want_bits=True, null_metric=False):
    """(rc, metric, bits or None, the refusal's message) of one harness run."""
    llr = np.ascontiguousarray(np.asarray(llr, dtype=np.float64).reshape(-1, N))
    B = len(llr)
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "result.bin")
    with open(case, "wb") as f:
        f.write(np.array([kind, N, K, B, int(want_bits), int(null_metric)], dtype="<i4").tobytes())
        f.write(np.ascontiguousarray(frozen, dtype="<i4").tobytes())
        f.write(np.ascontiguousarray(node_type, dtype="<i4").tobytes())
        f.write(llr.astype("<f8").tobytes())
    p = subprocess.run([exe, case, res], check=True, capture_output=True, text=True)
    raw = open(res, "rb").read()
    rc = int(np.frombuffer(raw[:4], dtype="<i4")[0])
    if rc:
        return rc, None, None, p.stdout.strip()
    metric = np.frombuffer(raw[4:4 + 8 * B], dtype="<f8")
    bits = np.frombuffer(raw[4 + 8 * B:], dtype=np.uint8).reshape(B, K) if want_bits else None
    assert len(raw) == 4 + 8 * B + (B * K if want_bits else 0)
    return rc, metric, bits, ""


def test_abi_declares_exports_and_binds_dmetric():
    from quantized_decoder_polar_codes_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "qpd.h")).read()
    # additive: the ABI version and the structs are what they were
    assert re.search(r"#define QPD_ABI_VERSION 7\b", hdr) and _lib.ABI_VERSION == 7
    assert ctypes.sizeof(_lib.QpdInfo) == 96 and ctypes.sizeof(_lib.QpdStatusArgs) == 32
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.EXPORTED
    assert "DMetric.cpp:24-177" in hdr
    so = os.path.join(ROOT, "quantized_decoder_polar_codes_amd", "libqpd.so")
    if os.path.exists(so):  # built: the symbols are exported (dlsym without initialising a device)
        L = ctypes.CDLL(so)
        for name in NEW_SYMBOLS:
            assert hasattr(L, name), name


def test_polarbd_exports_both_classes():
    import PolarBD
    from PolarBD.PolarBD.CASCLWithRNTI import CASCLDecoder  # noqa: F401
    from PolarBD.PolarBD.DMetricCalculator import DMetricCalculator

    assert PolarBD.PolarBD.DMetricCalculator.DMetricCalculator is DMetricCalculator
    assert "not provided" not in (PolarBD.__doc__ or "")


@pytest.mark.parametrize("path", DM_FILES, ids=lambda p: os.path.basename(p)[:-4])
def test_host_engine_reproduces_reference_dmetric(path, harness, tmp_path):
    g = load_golden(path)
    N, K = int(g["N"]), int(g["K"])
    rc, dm, bits, _ = host_dmetric(harness, tmp_path, QPD_FASTSC_FLOAT, N, K, g["frozen"], g["node_type"], g["llr"])
    assert rc == 0
    assert (dm == g["dmetric"]).all(), np.flatnonzero(dm != g["dmetric"])  # the same doubles
    assert (bits == dmetric_ref.dmetric(N, g["frozen"], g["node_type"], g["llr"])[1]).all()
    # the metric alone (NULL out): the same doubles
    rc, dm1, none, _ = host_dmetric(harness, tmp_path, QPD_FASTSC_FLOAT, N, K, g["frozen"], g["node_type"], g["llr"],
                                    want_bits=False)
    assert rc == 0 and none is None and (dm1 == g["dmetric"]).all()


def mask_frames(fm, B, seed):
    """B frames for the code of mask fm in the fixtures' three classes: f % 3 == 0 a codeword over AWGN at
    1.5 dB, 1 noise only, 2 LLRs from {-1, -0.5, 0, 0.5, 1}."""
    from quantized_decoder_polar_codes_amd import codes as C

    N, mb = fm.size, np.flatnonzero(fm == 0)
    K = mb.size
    rng = np.random.default_rng(seed)
    sigma = np.sqrt(1 / (2 * (K / N) * 10 ** (1.5 / 10)))
    x = C.polar_encode(rng.integers(0, 2, size=(B, K), dtype=np.uint8), mb, N)
    noise = rng.normal(0, sigma, size=(B, N))
    llr = ((1.0 - 2.0 * x) + noise) * 2 / sigma ** 2
    cls = np.arange(B) % 3
    llr[cls == 1] = (noise * 2 / sigma ** 2)[cls == 1]
    llr[cls == 2] = np.array([-1.0, -0.5, 0.0, 0.5, 1.0])[rng.integers(0, 5, size=(B, N))][cls == 2]
    return llr


def grid():
    """(N, mask name) over block and edge masks; a mask whose root is labelled (refused by qpd_create, the
    reference's depth -1 case) or that has no information bit is no code of this decoder."""
    out = []
    for N in (8, 16, 64, 256):
        names = ["block%d" % s for s in M.BLOCK_SEEDS.get(N, (3, 5, 8))[:3]] + list(M.EDGE_NAMES)
        for name in names:
            fm = M.named_mask(N, name)
            if (fm == 0).sum() and not M.special_root(fm, "FastSC-LUT"):
                out.append((N, name))
    return out


GRID = grid()


def test_grid_reaches_r0_and_rep_nodes_at_every_size():
    assert len(GRID) >= 24
    for N in (8, 16, 64, 256):
        kinds = {k for n, name in GRID if n == N for k, s in M.labelled_nodes(M.named_mask(N, name)) if s > 1}
        # the nodes the metric reads everywhere; the other two kinds where the masks are long enough for them
        assert ({"R0", "REP"} if N < 64 else {"R0", "REP", "R1", "SPC"}) <= kinds, (N, kinds)


@pytest.mark.parametrize("N,name", GRID, ids=lambda v: str(v))
def test_host_engine_matches_restatement_on_masks(N, name, harness, tmp_path):
    fm = M.named_mask(N, name)
    nt = M.node_type_of(fm)
    llr = mask_frames(fm, 12, 1000 + N)
    want_dm, want_bits = dmetric_ref.dmetric(N, fm, nt, llr)
    rc, dm, bits, _ = host_dmetric(harness, tmp_path, QPD_FASTSC_FLOAT, N, int((fm == 0).sum()), fm, nt, llr)
    assert rc == 0
    assert (dm == want_dm).all(), np.flatnonzero(dm != want_dm)
    assert (bits == want_bits).all()


def test_argument_checks(harness, tmp_path):
    g = load_golden(DM_FILES[-1])
    N, K = int(g["N"]), int(g["K"])
    args = (N, K, g["frozen"], g["node_type"], g["llr"][:2])
    for kind, name in ((QPD_SCL_FLOAT, "SCLDecoder"), (QPD_SC_LUT, "SCLUTDecoder"), (QPD_FASTSC_LUT, "FastSCLUTDecoder")):
        rc, _, _, msg = host_dmetric(harness, tmp_path, kind, *args)
        assert rc == QPD_E_INVALID and name in msg, (kind, msg)  # the message names the kind
    rc, _, _, msg = host_dmetric(harness, tmp_path, QPD_FASTSC_FLOAT, *args, null_metric=True)
    assert rc == QPD_E_INVALID and "metric" in msg
    rc, dm, bits, _ = host_dmetric(harness, tmp_path, QPD_FASTSC_FLOAT, *args, want_bits=False)  # NULL out is fine
    assert rc == 0 and bits is None and (dm == g["dmetric"][:2]).all()


def test_other_decoder_classes_refuse_in_python():
    from quantized_decoder_polar_codes_amd import decoders as D

    g = load_golden(DM_FILES[-1])
    for kind in ("SC", "SCL", "FastSCL"):
        dec = D.from_quant(kind, int(g["N"]), int(g["K"]), g["frozen"], L=4, node_type=g["node_type"], create=False)
        with pytest.raises(TypeError, match="FastSCDecoder"):  # before any C call: there is no handle
            dec.dmetric_batch(g["llr"])


@pytest.mark.gpu
@pytest.mark.host_engine
@pytest.mark.parametrize("path", DM_FILES[-2:], ids=lambda p: os.path.basename(p)[:-4])
def test_drop_in_calculator_returns_the_reference_double(path):
    from PolarBD.PolarBD.DMetricCalculator import DMetricCalculator

    g = load_golden(path)
    N = int(g["N"])
    calc = DMetricCalculator(N, int(g["K"]), g["frozen"], 1 - g["frozen"], g["node_type"])
    for f in range(6):
        a, b = calc.calculate(g["llr"][f]), calc.calculate(g["llr"][f][None])  # [N] and [1, N]
        assert isinstance(a, float) and a == g["dmetric"][f] and b == g["dmetric"][f]
        assert_engine(calc._dec, "host")
    calc._dec.set_host_engine("cpu")
    assert (calc.calculate_batch(g["llr"]) == g["dmetric"]).all()
    # keyword names of the reference (py_DMetric.cpp:13)
    kw = DMetricCalculator(N=N, K=int(g["K"]), frozen_bits=g["frozen"], message_bits=1 - g["frozen"],
                           node_type=g["node_type"])
    assert kw.calculate(llr=g["llr"][0]) == g["dmetric"][0]
