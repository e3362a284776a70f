"""FastSCL-LUT / CA-FastSCL-LUT with 9 <= L <= 16 on the fast engine (lane groups of
16: keep_all16 / select_survivors16 at the leaf forks, the REP nodes' 2L -> L step and
every R1 layer; R1 nodes with up to 15 layers; qpd_fast_fscl16.hip).

engine="auto" keeps these decoders on the generic engine (test_gpu_parity pins that);
every case here asks for engine="fast" and checks that the W16 plan ran (engine 2,
16 lanes per frame).  mink (FastSCLLUTDecoder.cpp:19-34) sorts 2L > 16 candidates at
each of its four call sites (:129 R1 layers, :187 REP, :256 / :332 leaves), and an R1
node of more than 16 elements sorts its magnitudes, with libstdc++'s introsort, which
is not stable: the bits depend on its exact steps wherever keys
tie, so the cases use tie-heavy tables (2 / 3 distinct magnitudes), exact-zero quanta,
the bench tables (one quanta row per node: the rank-in-record R1 path) and the
reference build's own goldens.

(512, 256, 16) of the shape list has an R1 node of 64 elements, which the W16 plan
does not serve by contract (r1_large is not extended): that shape checks the refusal
and the generic engine's bits, and (512, 200, 16) stands in for N = 512 on the plan.
"""
import dataclasses
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, assert_frames_equal, golden_packed, load_golden

gpu = pytest.mark.gpu

# N, K, L, distinct magnitudes
SHAPES = [(64, 32, 16, 3), (128, 64, 16, 2), (256, 128, 12, 3), (256, 100, 9, 3), (512, 256, 16, 3), (512, 200, 16, 2),
          (1024, 512, 16, 3), (1024, 512, 13, 3)]


@pytest.fixture(scope="module")
def qpd(native_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import quantized_decoder_polar_codes_amd as Q

    return Q


def _code(N, K):
    from quantized_decoder_polar_codes_amd import codes as C

    _, mb, fm, mm = C.construct_pw(N, K)
    return fm, C.identify_nodes(N, mb).astype(np.int32)


def _special_root(nt):
    return 0 <= nt[0] <= 2


def node_census(N, nt):
    """The ops a FastSCL plan without mixed bottom subtrees makes of a code: special
    nodes by type and size, plain height-3 subtrees (BOT3), as the host's fast_ops."""
    n = int(np.log2(N))
    out = {"R0": 0, "REP": 0, "R1<=16": 0, "R1 17-32": 0, "R1>32": 0, "BOT3": 0}

    def special(d, node):
        t = nt[(1 << d) + node - 1]
        return t if d < n and 0 <= t <= 2 else -1

    def walk(d, node):
        t = special(d, node)
        if t >= 0:
            size = N >> d
            out["R0" if t == 0 else "REP" if t == 2 else "R1<=16" if size <= 16 else "R1 17-32" if size <= 32 else "R1>32"] += 1
        elif d == n - 3 and all(special(dd, (node << (dd - d)) + k) < 0 for dd in range(d, n) for k in range(1 << (dd - d))):
            out["BOT3"] += 1
        elif d < n:
            walk(d + 1, 2 * node)
            walk(d + 1, 2 * node + 1)

    walk(0, 0)
    return out


def _served(N, K):
    fm, nt = _code(N, K)
    return not _special_root(nt) and node_census(N, nt)["R1>32"] == 0


def test_shapes_cover_every_op_class():
    """The shapes that run on the W16 plan hold, between them, R1 nodes of <= 16 and of
    17..32 elements, REP and R0 nodes and plain BOT3 subtrees (CPU: identify_nodes)."""
    total = {}
    ran = [(N, K) for N, K, L, mags in SHAPES if _served(N, K)]
    assert len(ran) >= len(SHAPES) - 1 and (1024, 512) in ran
    for N, K in ran:
        for k, c in node_census(N, _code(N, K)[1]).items():
            total[k] = total.get(k, 0) + c
    for cls in ("R1<=16", "R1 17-32", "REP", "R0", "BOT3"):
        assert total[cls] > 0, (cls, total)
    assert node_census(1024, _code(1024, 512)[1])["R1 17-32"] == 2  # the 5G code's two 32-element R1 nodes


def _frames(N, L, B):
    rng = np.random.default_rng(N * L)
    sym = rng.integers(0, 16, size=(B, N), dtype=np.int32)
    sym[: B // 4] = np.clip(sym[: B // 4] // 2 + 8, 0, 15)  # confident runs: long identity stretches
    sym[B // 4: B // 2] = 7  # all-equal symbols: every fork a tie
    return sym


def _fast(qpd, kind, p, K, fm, L, nt, **kw):
    dec = qpd.from_packed(kind, p, K, fm, L=L, node_type=nt, engine="fast", **kw)
    info = dec.info()
    assert info["engine"] == 2 and info["lanes_per_frame"] == 16, info
    return dec


def _refused_and_generic_decodes(qpd, oracle_mod, p, K, fm, L, nt, sym, label):
    """An unserved plan: the explicit request fails, AUTO decodes the oracle's bits on the generic engine."""
    with pytest.raises(ValueError, match="R1 node"):
        qpd.from_packed("FastSCL-LUT", p, K, fm, L=L, node_type=nt, engine="fast")
    dec = qpd.from_packed("FastSCL-LUT", p, K, fm, L=L, node_type=nt, engine="auto")
    assert dec.info()["engine"] == 1
    want = oracle_mod.decode_lut("FastSCL-LUT", p, K, L, fm, sym, node_type=nt)
    assert_frames_equal(dec.decode_batch(sym), want, dec, label)


@gpu
@pytest.mark.parametrize("N,K,L,mags", SHAPES)
def test_fastscl_w16_random_tables_vs_oracle(N, K, L, mags, qpd, oracle_mod):
    from quantized_decoder_polar_codes_amd import lut as LU

    p = LU.random_luts(N, 16, seed=N + L, distinct_mags=mags)
    fm, nt = _code(N, K)
    if _special_root(nt):
        pytest.skip("special root: rejected on both sides (test_gpu_parity)")
    sym = _frames(N, L, 40 if N >= 1024 else 160)
    if node_census(N, nt)["R1>32"]:
        _refused_and_generic_decodes(qpd, oracle_mod, p, K, fm, L, nt, sym[:40], f"fscl-w16-unserved-{N}-{K}-{L}")
        return
    dec = _fast(qpd, "FastSCL-LUT", p, K, fm, L, nt)
    want = oracle_mod.decode_lut("FastSCL-LUT", p, K, L, fm, sym, node_type=nt)
    redo = lambda rows: _fast(qpd, "FastSCL-LUT", p, K, fm, L, nt).decode_batch(sym[rows])  # noqa: E731
    assert_frames_equal(dec.decode_batch(sym), want, dec, f"fscl-w16-{N}-{K}-{L}-{mags}", redo, sym)


@gpu
@pytest.mark.parametrize("name", ["fastscllut_n128_k64_l16_random", "fastscllut_n1024_k512_l16_random"])
def test_fastscl_w16_reference_goldens(name, qpd):
    """Expected bits from the reference build itself."""
    g = load_golden(os.path.join(GOLDEN_DIR, name + ".npz"))
    N, K, L = int(g["N"]), int(g["K"]), int(g["L"])
    assert str(g["kind"]) == "FastSCL-LUT" and L == 16
    dec = _fast(qpd, "FastSCL-LUT", golden_packed(g), K, g["frozen"], L, g["node_type"])
    assert_frames_equal(dec.decode_batch(g["symbols"].astype(np.int32)), g["expected"], dec, f"fscl-w16-golden-{name}")


@gpu
@pytest.mark.parametrize("N,A,L", [(128, 40, 12), (128, 40, 16), (256, 100, 16)])
def test_ca_fastscl_w16_vs_oracle(N, A, L, qpd, oracle_mod):
    """Frames that carry a real CRC, so the CRC decides the output path (ca_winner on lane groups of 16)."""
    from quantized_decoder_polar_codes_amd import codes as C
    from quantized_decoder_polar_codes_amd import lut as LU

    K = A + 24
    _, mb, fm, mm = C.construct_pw(N, K)
    nt = C.identify_nodes(N, mb).astype(np.int32)
    assert not _special_root(nt)
    p = LU.random_luts(N, 16, seed=900 + N + L, distinct_mags=3)
    pm = LU.minsum_uniform_luts(N)
    rng = np.random.default_rng(N + A + L)
    B = 160
    msg = rng.integers(0, 2, size=(B, A), dtype=np.uint8)
    u = np.concatenate([msg, oracle_mod.crc_encode(msg)[:, : K - A]], axis=1)
    x = C.polar_encode(u, mb, N)
    sigma = np.sqrt(1 / (2 * (K / N) * 10 ** (1.0 / 10)))
    llr = ((1.0 - 2.0 * x) + rng.normal(0, sigma, size=(B, N))) * 2 / sigma ** 2
    sym = np.clip(np.rint(llr / 0.5 + 7.5), 0, 15).astype(np.int32)
    for tables, tag in ((pm, "minsum"), (p, "random")):
        dec = _fast(qpd, "CA-FastSCL-LUT", tables, K, fm, L, nt, A=A)
        assert dec.info()["out_bits"] == A
        want = oracle_mod.decode_lut_ca("CA-FastSCL-LUT", tables, K, A, L, fm, sym, node_type=nt)
        assert_frames_equal(dec.decode_batch(sym), want, dec, f"ca-fscl-w16-{N}-{A}-{L}-{tag}")


@gpu
def test_fastscl_w16_zero_quanta_ties(qpd, oracle_mod):
    """Exact-zero quanta: keep and flip of a path tie (kf == pm) -- at the leaves (row n-1),
    and in every row that an R1 / REP node reads (their layers' and 2L -> L steps' keep and
    flip tie)."""
    from quantized_decoder_polar_codes_amd import lut as LU

    N, K, L = 256, 128, 16
    n = 8
    p = LU.random_luts(N, 16, seed=77, distinct_mags=3)
    fm, nt = _code(N, K)
    depths = {d for d in range(1, n) for node in range(1 << d) if 0 <= nt[(1 << d) + node - 1] <= 2 and nt[(1 << d) + node - 1] != 0}
    assert depths, "the code has R1 / REP nodes"
    vcl = p.vcl.copy()
    vcl[n - 1][:, ::3] = 0.0  # leaf row n-1: a third of the symbols decide with |dm| = 0
    for d in sorted(depths):
        vcl[d - 1][:, 1::3] = 0.0  # the special nodes of depth d read row d-1 (H3)
    p = dataclasses.replace(p, vcl=vcl)
    sym = np.random.default_rng(3).integers(0, 16, size=(128, N), dtype=np.int32)
    dec = _fast(qpd, "FastSCL-LUT", p, K, fm, L, nt)
    want = oracle_mod.decode_lut("FastSCL-LUT", p, K, L, fm, sym, node_type=nt)
    assert_frames_equal(dec.decode_batch(sym), want, dec, "fscl-w16-zero-quanta")


@gpu
def test_fastscl_w16_schedule_switches(qpd, oracle_mod, monkeypatch):
    """One frame set, two, and two pointer words per path: the same bits."""
    from quantized_decoder_polar_codes_amd import lut as LU

    N, K, L = 256, 128, 16
    p = LU.random_luts(N, 16, seed=N + L + 1, distinct_mags=3)
    fm, nt = _code(N, K)
    sym = _frames(N, L, 160)
    want = oracle_mod.decode_lut("FastSCL-LUT", p, K, L, fm, sym, node_type=nt)
    for env, fpw in (({"QPD_SETS": "1"}, 4), ({"QPD_SETS": "2"}, 8), ({"QPD_NO_PW1": "1"}, 8)):
        for k in ("QPD_SETS", "QPD_NO_PW1"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        dec = _fast(qpd, "FastSCL-LUT", p, K, fm, L, nt)
        assert dec.info()["frames_per_wave"] == fpw
        if "QPD_NO_PW1" in env:
            assert dec.info()["fast_variant"] & 1 == 0
        assert_frames_equal(dec.decode_batch(sym), want, dec, f"fscl-w16-switch-{env}")


@gpu
def test_fastscl_w16_unserved_plan(qpd, oracle_mod, monkeypatch):
    """An R1 node of more than 16 elements without its LDS tail (here: no LDS rows at all):
    engine="fast" refuses, engine="auto" decodes the oracle's bits on the generic engine."""
    from quantized_decoder_polar_codes_amd import lut as LU

    N, K, L = 1024, 512, 16
    p = LU.random_luts(N, 16, seed=5, distinct_mags=3)
    fm, nt = _code(N, K)
    sym = _frames(N, L, 24)
    monkeypatch.setenv("QPD_LDS_BUDGET", "256")
    _refused_and_generic_decodes(qpd, oracle_mod, p, K, fm, L, nt, sym, "fscl-w16-unserved-lds")
    monkeypatch.delenv("QPD_LDS_BUDGET")
    _fast(qpd, "FastSCL-LUT", p, K, fm, L, nt)  # with its LDS tail the same code is served


@gpu
def test_fastscl_w16_bench_workload_vs_oracle_and_generic(qpd, oracle_mod):
    """The bench workload (MinDistortion tables: one quanta row per node, the R1 ranks in
    the op records; AWGN at 2 dB) at L = 16: the oracle on 96 frames, the generic engine on 2^14."""
    import bench

    wl = bench.workload(1024, 512, 16, "FastSCL-LUT", 1 << 14, 2.0)
    assert wl.dec.info()["engine"] == 1  # AUTO: the generic engine
    dec = _fast(qpd, "FastSCL-LUT", wl.packed, 512, wl.fm, 16, wl.nt)
    got = dec.decode_batch(wl.sym).cpu().numpy()
    sym = wl.sym.cpu().numpy()
    want = oracle_mod.decode_lut("FastSCL-LUT", wl.packed, 512, 16, wl.fm, sym[:96], node_type=wl.nt)
    assert_frames_equal(got[:96], want, dec, "fscl-w16-bench-oracle")
    ref = wl.dec.decode_batch(wl.sym).cpu().numpy()
    bad = np.flatnonzero((got != ref).any(1))
    assert bad.size == 0, f"{bad.size} of {len(got)} frames differ from the generic engine: {bad[:10]}"


@gpu
def test_fastscl_w16_noiseless_roundtrip(qpd):
    import torch

    from quantized_decoder_polar_codes_amd import codes as C
    from quantized_decoder_polar_codes_amd import lut as LU

    N, K, L = 1024, 512, 16
    _, mb, fm, mm = C.construct_pw(N, K)
    nt = C.identify_nodes(N, mb).astype(np.int32)
    rng = np.random.default_rng(11)
    msg = rng.integers(0, 2, size=(1 << 14, K), dtype=np.uint8)
    u = C.polar_encode(msg, mb, N)
    sym = np.where(u == 0, 15, 0).astype(np.int32)  # confident symbols of the right sign
    dec = _fast(qpd, "FastSCL-LUT", LU.minsum_uniform_luts(N), K, fm, L, nt)
    got = dec.decode_batch(torch.from_numpy(sym).cuda()).cpu().numpy()
    assert np.array_equal(got, msg)


@gpu
def test_fastscl_w16_input_flag(qpd, oracle_mod):
    """An out-of-range channel symbol is reported, and the flag is cleared for the next batch."""
    from quantized_decoder_polar_codes_amd import lut as LU

    N, K, L = 256, 128, 16
    p = LU.random_luts(N, 16, seed=9, distinct_mags=3)
    fm, nt = _code(N, K)
    sym = np.random.default_rng(9).integers(0, 16, size=(40, N), dtype=np.int32)
    want = oracle_mod.decode_lut("FastSCL-LUT", p, K, L, fm, sym, node_type=nt)
    dec = _fast(qpd, "FastSCL-LUT", p, K, fm, L, nt)
    wrong = sym.copy()
    wrong[20, N // 2 + 1] = 16  # a symbol of the root's second half
    with pytest.raises(ValueError):
        dec.decode_batch(wrong)
    assert_frames_equal(dec.decode_batch(sym), want, dec, "fscl-w16-after-flag")
