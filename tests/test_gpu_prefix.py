"""Frozen-prefix split (lut_prefix_kernel, csrc/qpd_fast.hip): SCL-LUT (and
CA-SCL-LUT) in pre-mode run the schedule up to the first information leaf once
per frame (stage 1), optionally to the second with 2 paths (stage 1b, L = 2,
QPD_PFX1B=1) and to the third with 4 (stage 2, L = 4); the decode kernel
resumes from the exported rows and path metrics.  The bits must equal the
oracle's and the unsplit kernel's (QPD_NO_PFX=1) on every input:
  * PW codes at the bench size (split present) and odd batch sizes;
  * codes whose first bit is information (a prefix of f ops only) or whose
    prefix is most of the schedule;
  * CRC-aided kinds, whose tail checks every path's CRC.
"""
import numpy as np
import pytest

from conftest import assert_frames_equal

pytestmark = pytest.mark.gpu

SPLIT = ("SCL-LUT",)  # the kinds that take the split (FastSCL's nodes already skip most of the prefix)


@pytest.fixture(scope="module")
def qpd(native_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import quantized_decoder_polar_codes_amd as Q

    return Q


def _code(N, K):
    from quantized_decoder_polar_codes_amd import codes as C

    _, mb, fm, _ = C.construct_pw(N, K)
    return fm, C.identify_nodes(N, mb).astype(np.int32)


def _tables(N, seed):
    from quantized_decoder_polar_codes_amd import lut as LU

    return LU.random_luts(N, 16, seed=seed, distinct_mags=3)


def _make(qpd, monkeypatch, kind, p, K, fm, L, nt, split, **kw):
    if split:
        monkeypatch.delenv("QPD_NO_PFX", raising=False)
    else:
        monkeypatch.setenv("QPD_NO_PFX", "1")
    return qpd.from_packed(kind, p, K, fm, L=L, node_type=nt, **kw)


@pytest.mark.parametrize("B", [24, 77])
@pytest.mark.parametrize("kind", ["SCL-LUT", "FastSCL-LUT"])
def test_prefix_matches_oracle(kind, B, qpd, oracle_mod, monkeypatch):
    N, K, L = 1024, 512, 8
    fm, nt = _code(N, K)
    p = _tables(N, 7000 + B)
    sym = np.random.default_rng(B).integers(0, 16, size=(B, N), dtype=np.int32)
    dec = _make(qpd, monkeypatch, kind, p, K, fm, L, nt, True)
    assert (dec.info()["prefix_ops"] > 0) == (kind in SPLIT)
    want = oracle_mod.decode_lut(kind, p, K, L, fm, sym, node_type=nt)
    assert_frames_equal(dec.decode_batch(sym), want, dec, f"prefix-{kind}-{B}")


@pytest.mark.parametrize("N,K,L", [(1024, 512, 8), (1024, 256, 4), (512, 400, 8), (256, 64, 2), (128, 96, 16)])
@pytest.mark.parametrize("kind", ["SCL-LUT", "FastSCL-LUT"])
def test_prefix_equals_unsplit(kind, N, K, L, qpd, monkeypatch):
    """Split and unsplit schedules give the same bits on noisy codewords and on
    random symbols (4099 frames: a partial last task in both kernels)."""
    import torch

    from quantized_decoder_polar_codes_amd import lut as LU

    fm, nt = _code(N, K)
    if kind == "FastSCL-LUT" and 0 <= nt[0] <= 2:
        pytest.skip("special root: undefined in the reference")
    p = LU.minsum_uniform_luts(N)
    rng = np.random.default_rng(N + K + L)
    sym = rng.integers(0, 16, size=(4099, N), dtype=np.int32)
    sym[: 2048] = np.clip(sym[: 2048] // 2 + 8, 0, 15)  # a biased half: long runs of confident symbols
    a = _make(qpd, monkeypatch, kind, p, K, fm, L, nt, True)
    b = _make(qpd, monkeypatch, kind, p, K, fm, L, nt, False)
    assert b.info()["prefix_ops"] == 0
    if L <= 8:
        assert (a.info()["prefix_ops"] > 0) == (kind in SPLIT)
    st = torch.from_numpy(sym).cuda()
    ga, gb = a.decode_batch(st).cpu().numpy(), b.decode_batch(st).cpu().numpy()
    assert np.array_equal(ga, gb), np.flatnonzero((ga != gb).any(1))[:10]


@pytest.mark.parametrize("N,K,L", [(1024, 512, 8), (512, 256, 8), (1024, 384, 6)])
def test_prefix_stage1b(N, K, L, qpd, oracle_mod, monkeypatch):
    """Stage 1b (2 live paths at L = 2) on tie-heavy tables (3 distinct quanta
    magnitudes, all-equal symbol frames: the L = 2 forks see tied keeps and
    flips): the bits equal the default split (no stage 1b), the unsplit kernel
    and the oracle."""
    fm, nt = _code(N, K)
    p = _tables(N, 500 + N + K + L)
    rng = np.random.default_rng(N * K + L)
    sym = rng.integers(0, 16, size=(2053, N), dtype=np.int32)
    sym[:256] = 7
    sym[256:1024] = np.clip(sym[256:1024] // 2 + 8, 0, 15)
    monkeypatch.setenv("QPD_PFX1B", "1")
    a = _make(qpd, monkeypatch, "SCL-LUT", p, K, fm, L, nt, True)
    monkeypatch.delenv("QPD_PFX1B", raising=False)
    c = _make(qpd, monkeypatch, "SCL-LUT", p, K, fm, L, nt, True)
    b = _make(qpd, monkeypatch, "SCL-LUT", p, K, fm, L, nt, False)
    assert a.info()["prefix_ops"] > c.info()["prefix_ops"] > 0 == b.info()["prefix_ops"]  # stage 1b taken
    ga, gc, gb = a.decode_batch(sym), c.decode_batch(sym), b.decode_batch(sym)
    assert np.array_equal(ga, gc), np.flatnonzero((ga != gc).any(1))[:10]
    assert np.array_equal(ga, gb), np.flatnonzero((ga != gb).any(1))[:10]
    rows = np.r_[0:40, 256:296, 1024:1064]
    want = oracle_mod.decode_lut("SCL-LUT", p, K, L, fm, sym[rows], node_type=nt)
    assert_frames_equal(ga[rows], want, a, f"prefix-1b-{N}-{K}-{L}")


def test_prefix_all_stages_grown_records(qpd, oracle_mod, monkeypatch):
    """Stages 1, 1b and 2 on one handle, 64 frames and then 4096: the second call
    reallocates every stage's record buffer, so the import ops of stage 1b, stage 2
    and the decode kernel are patched again, each to its own stage's new buffer.
    N = 128, K = 48: the smallest PW code at L = 8 whose plan puts ops in all three
    stages (the plan compiler on the CPU: 7 / 12 / 10 ops; K = 64 gets no stage 1b)."""
    N, K, L = 128, 48, 8
    fm, nt = _code(N, K)
    p = _tables(N, 1248)
    sym = np.random.default_rng(1248).integers(0, 16, size=(4096, N), dtype=np.int32)
    sym[:1024] = np.clip(sym[:1024] // 2 + 8, 0, 15)
    monkeypatch.setenv("QPD_PFX1B", "1")
    a = _make(qpd, monkeypatch, "SCL-LUT", p, K, fm, L, nt, True)
    monkeypatch.delenv("QPD_PFX1B", raising=False)
    c = _make(qpd, monkeypatch, "SCL-LUT", p, K, fm, L, nt, True)
    assert a.info()["prefix_ops"] > c.info()["prefix_ops"] > 0  # stage 1b taken
    want = oracle_mod.decode_lut("SCL-LUT", p, K, L, fm, sym, node_type=nt)
    assert_frames_equal(a.decode_batch(sym[:64]), want[:64], a, "prefix-grow-64")
    assert_frames_equal(a.decode_batch(sym), want, a, "prefix-grow-4096")


@pytest.mark.parametrize("N,K", [(64, 64), (1024, 1024), (1024, 16)])
def test_prefix_edge_codes_exact(N, K, qpd, oracle_mod, monkeypatch):
    """Every bit information (K = N: the prefix is only the f ops down to the
    first leaf) or a long prefix (K = 16 of 1024: stage 1 runs most of the
    schedule): whatever the plan chose, the bits are the oracle's."""
    fm, nt = _code(N, K)
    p = _tables(N, 31 + K)
    sym = np.random.default_rng(K).integers(0, 16, size=(40, N), dtype=np.int32)
    dec = _make(qpd, monkeypatch, "SCL-LUT", p, K, fm, 8, nt, True)
    want = oracle_mod.decode_lut("SCL-LUT", p, K, 8, fm, sym, node_type=nt)
    assert_frames_equal(dec.decode_batch(sym), want, dec, f"prefix-edge-{N}-{K}")


@pytest.mark.parametrize("kind", ["CA-SCL-LUT", "CA-FastSCL-LUT"])
def test_prefix_crc_aided(kind, qpd, monkeypatch):
    N, A, K, L = 1024, 500, 512, 8
    fm, nt = _code(N, K)
    p = _tables(N, 99)
    sym = np.random.default_rng(5).integers(0, 16, size=(24, N), dtype=np.int32)
    a = _make(qpd, monkeypatch, kind, p, K, fm, L, nt, True, A=A)
    b = _make(qpd, monkeypatch, kind, p, K, fm, L, nt, False, A=A)
    assert (a.info()["prefix_ops"] > 0) == (kind[3:] in SPLIT)
    ga = a.decode_batch(sym)
    assert np.array_equal(ga, b.decode_batch(sym))


@pytest.mark.parametrize("scale", ["below", "above"])
def test_prefix_guard_near_dbl_max_quanta(scale, qpd, oracle_mod):
    """Leaf quanta near DBL_MAX: path metrics may overflow to +inf, where the
    split's dead-slot seeding (path 0's rows) would differ from the reference's
    copies of other dead paths.  Quanta up to DBL_MAX / 2N keep every metric
    finite and take the split; larger ones decode unsplit.  Either way the bits
    are the oracle's, on the kernels and on the host engine."""
    from quantized_decoder_polar_codes_amd import lut as LU

    N, K, L = 1024, 512, 8
    n = 10
    fm, nt = _code(N, K)
    p = _tables(N, 4242)
    vcl = p.vcl.copy()
    bound = np.finfo(np.float64).max / (2 * N)
    top = np.abs(vcl[n - 1]).max()
    vcl[n - 1] *= (0.999 * bound if scale == "below" else 64 * bound) / top
    assert np.isfinite(vcl).all()
    q = LU.PackedLUT(N=p.N, v=p.v, lut_f=p.lut_f, f_base=p.f_base, f_step=p.f_step, lut_g=p.lut_g, g_base=p.g_base,
                     g_step=p.g_step, vcl=np.ascontiguousarray(vcl))
    sym = np.random.default_rng(8).integers(0, 16, size=(48, N), dtype=np.int32)
    dec = qpd.from_packed("SCL-LUT", q, K, fm, L=L)
    assert (dec.info()["prefix_ops"] > 0) == (scale == "below")
    want = oracle_mod.decode_lut("SCL-LUT", q, K, L, fm, sym)
    assert_frames_equal(dec.decode_batch(sym), want, dec, f"prefix-dblmax-{scale}")
    dec.set_host_engine("cpu")
    assert_frames_equal(dec.decode_batch(sym), want, dec, f"prefix-dblmax-{scale}-host", engine="host")
