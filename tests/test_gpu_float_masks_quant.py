"""GPU parity of the nine float-domain kinds (generic_decode_kernel<family,
DOM_FLOAT | DOM_UNIFORM | DOM_LLOYD>) on the inputs of tests/float_cases.py:
frozen masks no reliability order gives (R1 before R0, information at
position 0, a frozen last position, SPC and R1 nodes of every size, the
64-element R1 argsort on fp64 keys that tie), uniform re-quantizers whose
clip level and cell edges the values hit exactly at v = 2 .. 16 and at the
int32 limits, a step whose quotients only a correctly rounded division
floors right, ragged and unsorted Lloyd tables.

* every case against the CPU oracle, bit-exact (the oracle is pinned to the
  reference on the same grid by test_float_oracle_masks_quant.py and by the
  committed fixtures);
* decode status of the list kinds, CA-SCL also under a CRC mask;
* the device-tensor path and the fused Monte-Carlo path on grid quantizers;
* L = 32 on the wide instantiation;
* a Lloyd reconstruction list one short of its cells: reported, not read.
"""
import numpy as np
import pytest

import float_cases as F
from conftest import assert_engine

pytestmark = pytest.mark.gpu

GENERIC = 1  # qpd_info.engine


@pytest.fixture(scope="module")
def qpd(native_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import quantized_decoder_polar_codes_amd as Q

    return Q


def decoder_of(c, **kw):
    from quantized_decoder_polar_codes_amd.decoders import from_quant

    fm, nt, K = F.code_of(c.N, c.mask)
    return from_quant(c.kind, c.N, K, fm, L=c.L, node_type=nt, quant=F.quant_of(c), **F.decoder_kw(c), **kw)


def frames_differ(got, want):
    bad = np.flatnonzero((np.asarray(got) != np.asarray(want)).any(1))
    return bad, f"{bad.size}/{len(want)} frames differ, first {bad[:5]}"


@pytest.mark.parametrize("c", F.cases(), ids=lambda c: c.id)
def test_gpu_float_grid_matches_oracle(c, qpd, oracle_mod):
    if c.refused:  # a labelled root: undefined behaviour in the reference, both sides refuse
        with pytest.raises(RuntimeError):
            F.reference(c)
        with pytest.raises(ValueError):
            decoder_of(c)
        return
    dec = decoder_of(c)
    got = dec.decode_batch(F.frames_of(c))
    assert_engine(dec, "gpu")
    want = F.reference(c)
    assert got.shape == want.shape
    bad, msg = frames_differ(got, want)
    assert bad.size == 0, msg
    if c.L == 32:  # the wide list instantiation: 32 lanes per frame, two frames per wave
        info = dec.info()
        assert (info["engine"], info["lanes_per_frame"], info["frames_per_wave"]) == (GENERIC, 32, 2)


@pytest.mark.parametrize("c", F.status_cases(), ids=lambda c: c.id)
def test_gpu_float_grid_status(c, qpd, oracle_mod):
    """The output path's metric is the oracle's double, the CRC verdict is equal; CA-SCL also under a mask."""
    dec = decoder_of(c)
    x = F.frames_of(c)
    rows = np.arange(len(x))
    ca = c.kind == "CA-SCL"
    for mb in ((0, 1, F.ca_of(c)[1]) if ca else (0,)):
        bits, pml, winner, passed = F.reference_status(c, mb)
        got, st = dec.decode_batch(x, return_status=True, crc_mask=F.crc_mask(mb) if mb else None)
        assert_engine(dec, "gpu")
        bad, msg = frames_differ(got, bits)
        assert bad.size == 0, f"mask {mb}: {msg}"
        m = np.asarray(st.metric)
        bad = np.flatnonzero(m != pml[rows, winner])
        assert bad.size == 0, f"mask {mb}: metric of {bad.size} frames differs, first {bad[:4]}: {m[bad[:4]]}"
        if ca:
            assert (np.asarray(st.crc_pass) == passed).all(), f"mask {mb}: verdict"
        else:
            assert st.crc_pass is None
    if ca:  # the mask is not idle: it changes the winner or the verdict of some frame
        a, b = F.reference_status(c, 0), F.reference_status(c, 1)
        assert ((a[2] != b[2]) | (a[3] != b[3])).any()


DEVICE_CASES = [F.Case("SCL-Uniform", 64, "block6", 8, ("grid", 49.0 / 64.0, 15), 201),
                F.Case("SC-Lloyd", 64, "info0", 1, ("unsorted", 7), 202)]


@pytest.mark.parametrize("c", DEVICE_CASES, ids=lambda c: c.id)
def test_gpu_float_grid_device_tensor(c, qpd, oracle_mod):
    import torch

    dec = decoder_of(c)
    dev = dec.decode_batch(torch.from_numpy(np.array(F.frames_of(c))).cuda())
    torch.cuda.synchronize()
    assert dev.is_cuda
    bad, msg = frames_differ(dev.cpu().numpy(), F.reference(c))
    assert bad.size == 0, msg


@pytest.mark.parametrize("c", DEVICE_CASES, ids=lambda c: c.id)
def test_gpu_float_grid_monte_carlo(c, qpd, oracle_mod):
    """qpd_mc_decode_f64 with a channel quantizer whose reconstruction values lie on the decoder's grid: its
    bits and counters are those of decode_batch on the same frames, and the oracle's."""
    import torch

    from quantized_decoder_polar_codes_amd import montecarlo as MC

    dec = decoder_of(c)
    fm, nt, K = F.code_of(c.N, c.mask)
    edges, lut = MC.uniform_channel_quantizer(16, 0.5)
    rec = c.step * np.arange(-8, 8, dtype=np.float64)  # integer multiples of the step
    src = MC.GpuLlrFrames(dec, MC.sigma_for(2.0, K / c.N), 77, edges, lut, 16, rec=rec)
    msg_a, llr = src(1000, 200)
    bits_a = dec.decode_batch(llr)
    counts = torch.zeros(2, dtype=torch.int64, device=src.device)
    msg_b, bits_b = src.decode_frames(1000, 200, counts=counts)
    torch.cuda.synchronize()
    x = llr.cpu().numpy()
    assert np.isin(x, rec).all() and len(np.unique(x)) == 16
    assert torch.equal(msg_a, msg_b) and torch.equal(bits_a, bits_b)
    diff = bits_a != msg_a
    assert counts.tolist() == [int(diff.sum()), int(diff.any(1).sum())]
    want = oracle_mod.decode_float(c.kind, c.N, K, fm, x, L=c.L, node_type=nt, quant=F.quant_of(c))
    bad, msg = frames_differ(bits_b.cpu().numpy(), want)
    assert bad.size == 0, msg


@pytest.mark.parametrize("kind,L", [("SC-Lloyd", 1), ("SCL-Lloyd", 4)])
def test_gpu_short_reconstruction_list_is_reported(kind, L, qpd, oracle_mod):
    """A reconstruction list one short of its cells: a value in the top cell would read past the list (undefined
    in the reference).  q_lloyd sets the error word and uses 0.0 before any read; values below decode, and the
    word is cleared for the next call."""
    from quantized_decoder_polar_codes_amd.decoders import from_quant

    N = 64
    fm, nt, K = F.code_of(N, "random")
    q, top, below = F.short_rec_lloyd(N, 3)
    dec = from_quant(kind, N, K, fm, L=L, quant=q)
    want = oracle_mod.decode_float(kind, N, K, fm, below, L=L, quant=q)
    assert np.array_equal(dec.decode_batch(below), want)
    with pytest.raises(ValueError, match="Lloyd"):
        dec.decode_batch(top)
    assert_engine(dec, "gpu")
    assert np.array_equal(dec.decode_batch(below), want)  # flag cleared
