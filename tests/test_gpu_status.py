"""Decode status on the kernels (qpd_decode_status, include/qpd.h): the output
path's metric, the CRC verdict and the CRC mask, on the fast engine (the ST
instantiations of lut_fast_kernel), the generic engine and, next to them, the host
engine behind the same C-ABI.

* the reference's float CA-SCL with RNTI (tests/golden/bd/bd_*.npz) on
  QPD_CASCL_FLOAT, and through the PolarBD drop-in, exactly;
* SCL-LUT / CA-SCL-LUT against tests/status_ref.py (checked against the reference's
  fixtures in tests/test_status_host.py) on both engines, with and without a mask;
* L = 16 (lane groups of 16) and CA-FastSCL-LUT: the engines against each other,
  and CA-FastSCL-LUT against the plain FastSCL-LUT decoder of the same tables;
* partial blocks and canaries, optional outputs, the Python call, two streams.

These are fixtures at N = 64 and 128.  Every other status instantiation (the split
tail at N >= 256, lane groups of 2 .. 16, both pointer-word layouts, the R1L
twins, the planner's modes, launch seams, the wide generic kernel, the float list
kinds) is compared with the CPU oracle's status in tests/test_gpu_status_sweep.py.
There FastSCL-LUT, CA-FastSCL-LUT, L > 8 and float SCL / FastSCL rest on the oracle
and the host engine agreeing (tests/test_oracle_status.py), not on a recorded
reference value; SCL-Uniform and SCL-Lloyd, which the host engine does not decode,
rest on the oracle alone.
"""
import ctypes
import glob
import os

import numpy as np
import pytest

import status_ref
from conftest import GOLDEN_DIR, assert_engine, golden_packed, load_golden

pytestmark = pytest.mark.gpu

BD_FILES = sorted(glob.glob(os.path.join(GOLDEN_DIR, "bd", "bd_*.npz")))
MASK16 = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 1, 0, 1], dtype=np.uint8)
FAST, GENERIC = 2, 1  # qpd_info.engine
LUT_CASES = [("scllut_n128_k64_l8_random", None), ("ca_scllut_n128_a40_l8_minsum", 40)]


@pytest.fixture(scope="module")
def qpd(native_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import quantized_decoder_polar_codes_amd as Q

    return Q


def golden(name):
    return load_golden(os.path.join(GOLDEN_DIR, name + ".npz"))


def lut_decoder(g, kind, engine, A=None):
    from quantized_decoder_polar_codes_amd import decoders as D

    dec = D.from_packed(kind, golden_packed(g), int(g["K"]), g["frozen"], L=int(g["L"]), node_type=g["node_type"],
                        engine=engine, **({"A": A} if A else {}))
    assert dec.info()["engine"] == {"fast": FAST, "generic": GENERIC}[engine]
    return dec


def dev_status(dec, x, mask=None, metric=True, crc_pass=True, B=None, size=None, stream=None):
    """qpd_decode_status as a C caller: (bits, metric, pass) device tensors of `size` frames
    (default B), pre-filled with canaries (bits 0xEE, metric -7.0, pass 0x55)."""
    import torch

    from quantized_decoder_polar_codes_amd import _lib

    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    ty = {torch.int32: _lib.QPD_IN_I32, torch.uint8: _lib.QPD_IN_U8, torch.float64: _lib.QPD_IN_F64}[t.dtype]
    B = t.shape[0] if B is None else B
    size = B if size is None else size
    out = torch.full((size, dec.out_bits), 0xEE, dtype=torch.uint8, device=t.device)
    m = torch.full((size,), -7.0, dtype=torch.float64, device=t.device)
    ok = torch.full((size,), 0x55, dtype=torch.uint8, device=t.device)
    sa = _lib.QpdStatusArgs()
    if mask is not None:
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        sa.crc_mask, sa.crc_mask_bits = mask.ctypes.data, len(mask)
    if metric:
        sa.metric = m.data_ptr()
    if crc_pass:
        sa.crc_pass = ok.data_ptr()
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    _lib.check(_lib.load().qpd_decode_status(dec._h, ctypes.c_void_p(t.data_ptr()), ty, B, ctypes.c_void_p(out.data_ptr()),
                                             ctypes.byref(sa), ctypes.c_void_p(st)))
    return out, m, ok


def np3(r):
    import torch

    torch.cuda.synchronize()
    return tuple(a.cpu().numpy() for a in r)


def host_engine_status(dec, x, mask=None):
    """The same decoder's host engine through qpd_decode_status_host: (bits, metric, pass)."""
    dec.set_host_engine("cpu")
    try:
        bits, st = dec.decode_batch(np.asarray(x), return_status=True, crc_mask=mask)
        assert_engine(dec, "host")
    finally:
        dec.set_host_engine("gpu")
    return bits, st.metric, None if st.crc_pass is None else st.crc_pass.astype(np.uint8)


def bd_groups(g):
    groups = {}
    for f in range(len(g["llr"])):
        groups.setdefault(tuple(g["rnti"][f, : g["rnti_len"][f]].tolist()), []).append(f)
    return [(np.array(k, dtype=np.uint8), np.array(v)) for k, v in groups.items()]


# -- the reference's CASCLWithRNTI ------------------------------------------------------------------------

@pytest.mark.parametrize("path", BD_FILES, ids=lambda p: os.path.basename(p)[:-4])
def test_bd_fixture_on_the_kernels(path, qpd):
    import torch

    from quantized_decoder_polar_codes_amd.decoders import from_quant

    g = load_golden(path)
    dec = from_quant("CA-SCL", int(g["N"]), int(g["K"]), g["frozen"], L=int(g["L"]), A=int(g["A"]),
                     crc_n=int(g["crc_n"]), crc_loc=g["crc_loc"])
    for mask, idx in bd_groups(g):
        bits, st = dec.decode_batch(torch.from_numpy(g["llr"][idx]).cuda(), return_status=True,
                                    crc_mask=mask if len(mask) else None)
        assert_engine(dec, "gpu")
        assert bits.is_cuda and st.metric.is_cuda and st.crc_pass.is_cuda and st.crc_pass.dtype == torch.bool
        assert (bits.cpu().numpy() == g["bits"][idx]).all()
        assert (st.crc_pass.cpu().numpy() == g["is_pass"][idx]).all()
        assert (st.metric.cpu().numpy() == g["pm"][idx]).all()  # the same doubles


@pytest.mark.parametrize("path", BD_FILES, ids=lambda p: os.path.basename(p)[:-4])
def test_bd_fixture_through_the_polarbd_shim(path, qpd):
    from PolarBD.PolarBD.CASCLWithRNTI import CASCLDecoder

    g = load_golden(path)
    fm = g["frozen"]
    d = CASCLDecoder(int(g["N"]), int(g["K"]), int(g["A"]), int(g["L"]), fm.tolist(), (1 - fm).tolist(), int(g["crc_n"]),
                     g["crc_loc"].tolist())
    for f in range(len(g["llr"])):  # one decode(llr, RNTI) call per frame, as the reference is driven
        bits, pm, ok = d.decode(g["llr"][f][None], g["rnti"][f, : g["rnti_len"][f]].astype(np.int32))
        assert bits.dtype == np.uint8 and isinstance(pm, float) and isinstance(ok, bool)
        assert (bits == g["bits"][f]).all() and ok == bool(g["is_pass"][f]) and pm == float(g["pm"][f]), f
    assert_engine(d, "gpu")  # (QPD_HOST_ENGINE=gpu in the gpu tests: the one-frame call ran the kernels)


# -- SCL-LUT / CA-SCL-LUT against the restatement ---------------------------------------------------------

@pytest.fixture(scope="module")
def lut_refs():
    refs = {}
    for name, A in LUT_CASES:
        g = golden(name)
        for masked in ((False, True) if A else (False,)):
            refs[name, masked] = status_ref.decode(golden_packed(g), g["frozen"], int(g["L"]), g["symbols"], A=A,
                                                   mask=MASK16 if masked else None)
    return refs


@pytest.mark.parametrize("engine", ["fast", "generic"])
@pytest.mark.parametrize("name,A,masked", [LUT_CASES[0] + (False,), LUT_CASES[1] + (False,), LUT_CASES[1] + (True,)])
def test_lut_status_matches_restatement(name, A, masked, engine, qpd, lut_refs):
    g = golden(name)
    bits, pml, win, passed = lut_refs[name, masked]
    dec = lut_decoder(g, "CA-SCL-LUT" if A else "SCL-LUT", engine, A)
    got, m, ok = np3(dev_status(dec, g["symbols"].astype(np.int32), mask=MASK16 if masked else None, crc_pass=bool(A)))
    assert_engine(dec, "gpu")
    assert (got == bits).all()
    assert (m == pml[np.arange(len(win)), win]).all()
    if A:
        assert (ok == passed).all()
    if not masked:
        assert (got == g["expected"]).all()


# -- engines against each other ---------------------------------------------------------------------------

def three_engines(g, kind, A, x, mask):
    out = {}
    for engine in ("fast", "generic"):
        dec = lut_decoder(g, kind, engine, A)
        out[engine] = np3(dev_status(dec, x, mask=mask))
        assert_engine(dec, "gpu")
    out["host"] = host_engine_status(dec, x, mask)
    for other in ("generic", "host"):
        for a, b, what in zip(out["fast"], out[other], ("bits", "metric", "pass")):
            assert (a == b).all(), f"fast vs {other}: {what}"
    return out["fast"]


@pytest.mark.parametrize("masked", [False, True])
def test_l16_lane_groups_of_16(masked, qpd):
    g = golden("ca_scllut_n128_a40_l16_random")
    assert int(g["L"]) == 16
    bits, m, ok = three_engines(g, "CA-SCL-LUT", int(g["A"]), g["symbols"].astype(np.int32), MASK16 if masked else None)
    if not masked:
        assert (bits == g["expected"]).all()


def test_ca_fastscl_engines_and_plain_decoder(qpd):
    """CA-FastSCL-LUT has no restatement: the engines against each other, and the verdicts against
    the plain FastSCL-LUT decoder of the same code and tables (its K bits are reference-exact):
    m0 its metric, c0 the CRC of its K bits, computed here."""
    from quantized_decoder_polar_codes_amd import montecarlo as MC

    g = golden("ca_fastscllut_n128_a40_l8_minsum")
    N, K, A = int(g["N"]), int(g["K"]), int(g["A"])
    ca = lut_decoder(g, "CA-FastSCL-LUT", "fast", A)
    # more failing frames than the fixture holds: the library's generator at 0 dB, a fixed seed
    edges, lut = MC.uniform_channel_quantizer(16, 0.5)
    _, extra = MC.GpuFrames(ca, edges, lut, 16, MC.sigma_for(0.0, K / N), seed=20261)(0, 192)
    x = np.concatenate([g["symbols"].astype(np.int32), extra.cpu().numpy()])
    bits, m, ok = three_engines(g, "CA-FastSCL-LUT", A, x, None)
    plain = lut_decoder(g, "FastSCL-LUT", "fast")
    b0, m0, _ = np3(dev_status(plain, x, crc_pass=False))
    c0 = np.array([(status_ref.crc_check_code(r[:A])[: K - A] == r[A:K]).all() for r in b0])
    assert (m >= m0).all()
    fail, same = ok == 0, (ok == 1) & (m == m0)
    print(f"frames: {len(x)}, pass=0: {fail.sum()}, pass=1 at m0: {same.sum()}, pass=1 above m0: {((ok == 1) & (m > m0)).sum()}")
    assert fail.sum() >= 8 and same.sum() >= 8, "uninformative"
    assert (m[fail] == m0[fail]).all() and not c0[fail].any()
    # metric = m0 with c0 failing is a tie at the minimum: minsum tables give equal metrics, the plain
    # decoder outputs the first path at m0 and the CRC-aided one a later path at m0 that passes.  Shown
    # per such frame: under the mask that makes the plain winner's own check bits pass, the CRC-aided
    # decoder returns exactly that path -- it is its rank 0, at m0.
    tie = same & ~c0
    print(f"ties at m0: {tie.sum()}")
    assert tie.sum() * 10 <= same.sum(), "ties are the exception"
    for f in np.flatnonzero(tie):
        mask = status_ref.crc_check_code(b0[f, :A]) ^ b0[f, A:K]
        tb, tm, tok = np3(dev_status(ca, x[f:f + 1], mask=mask))
        assert (tb[0] == b0[f, :A]).all() and tm[0] == m0[f] and tok[0] == 1, f
    same = same & c0
    assert same.sum() >= 8 and (bits[same] == b0[same][:, :A]).all()
    assert not c0[(ok == 1) & (m > m0)].any()


# -- partial blocks, optional outputs, the Python call, streams ---------------------------------------------

@pytest.mark.parametrize("engine", ["fast", "generic"])
def test_partial_block_leaves_the_rest_untouched(engine, qpd):
    g = golden("ca_scllut_n128_a40_l8_minsum")
    dec = lut_decoder(g, "CA-SCL-LUT", engine, 40)
    assert 37 % dec.info()["frames_per_wave"] != 0
    x = g["symbols"].astype(np.int32)[:64]
    full = np3(dev_status(dec, x, mask=MASK16))
    part = np3(dev_status(dec, x, mask=MASK16, B=37, size=64))
    for a, b, canary in zip(part, full, (0xEE, -7.0, 0x55)):
        assert (a[:37] == b[:37]).all()
        assert (a[37:] == canary).all()


@pytest.mark.parametrize("engine", ["fast", "generic"])
def test_outputs_are_optional(engine, qpd):
    import torch

    g = golden("ca_scllut_n128_a40_l8_minsum")
    dec = lut_decoder(g, "CA-SCL-LUT", engine, 40)
    x = torch.from_numpy(g["symbols"].astype(np.int32)).cuda()
    bits, m, ok = np3(dev_status(dec, x))
    b1, m1, ok1 = np3(dev_status(dec, x, crc_pass=False))
    b2, m2, ok2 = np3(dev_status(dec, x, metric=False))
    b3, m3, ok3 = np3(dev_status(dec, x, metric=False, crc_pass=False))
    plain = dec.decode_batch(x).cpu().numpy()
    assert (b1 == bits).all() and (m1 == m).all() and (ok1 == 0x55).all()
    assert (b2 == bits).all() and (m2 == -7.0).all() and (ok2 == ok).all()
    assert (b3 == plain).all() and (m3 == -7.0).all() and (ok3 == 0x55).all()
    assert (bits == plain).all()  # no mask: the bits of the plain call


def test_decode_batch_status_from_uint8_cuda(qpd):
    import torch

    g = golden("ca_scllut_n128_a40_l8_minsum")
    dec = lut_decoder(g, "CA-SCL-LUT", "fast", 40)
    x = torch.from_numpy(g["symbols"].astype(np.uint8)).cuda()
    bits, st = dec.decode_batch(x, return_status=True)
    info = dec.info()
    assert info["u8_staged"] == 0 and info["last_engine"] == 1  # read as they are (pre-mode), on the kernels
    assert bits.is_cuda and st.metric.is_cuda and st.metric.dtype == torch.float64 and st.crc_pass.dtype == torch.bool
    want = np3(dev_status(dec, x.to(torch.int32)))
    assert (bits.cpu().numpy() == want[0]).all() and (st.metric.cpu().numpy() == want[1]).all()
    assert (st.crc_pass.cpu().numpy() == want[2].astype(bool)).all()
    assert (bits.cpu().numpy() == g["expected"]).all()
    # numpy in, numpy out; a decoder without CRC has no verdict
    nb, nst = dec.decode_batch(g["symbols"].astype(np.uint8), return_status=True)
    assert isinstance(nb, np.ndarray) and (nb == want[0]).all() and (nst.metric == want[1]).all()
    scl = lut_decoder(golden(LUT_CASES[0][0]), "SCL-LUT", "fast")
    _, sst = scl.decode_batch(golden(LUT_CASES[0][0])["symbols"], return_status=True)
    assert sst.crc_pass is None and sst.metric.shape == (len(golden(LUT_CASES[0][0])["symbols"]),)
    with pytest.raises(ValueError):
        scl.decode_batch(golden(LUT_CASES[0][0])["symbols"], return_status=True, crc_mask=MASK16)


def test_second_stream_right_after_the_first(qpd):
    import torch

    g = golden("ca_scllut_n128_a40_l8_minsum")
    dec = lut_decoder(g, "CA-SCL-LUT", "fast", 40)
    x = torch.from_numpy(g["symbols"].astype(np.int32)).cuda()
    serial_a = np3(dev_status(dec, x))
    serial_b = np3(dev_status(dec, x, mask=MASK16))
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    ra = dev_status(dec, x, stream=s1.cuda_stream)
    rb = dev_status(dec, x, mask=MASK16, stream=s2.cuda_stream)  # no wait in between: the library orders them
    for got, want in ((np3(ra), serial_a), (np3(rb), serial_b)):
        for a, b in zip(got, want):
            assert (a == b).all()
