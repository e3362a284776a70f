"""GPU parity: libqpd.so kernels vs the reference's decoded bits.

* golden vectors (reference outputs, tests/golden) -- bit-exact;
* the CPU oracle on seeded random inputs across N, K, L, kinds and table
  layouts, including tie-heavy tables (hazard H1), exact-zero quanta (H4),
  per-element tables and non-power-of-two list sizes -- bit-exact;
* size-independent properties at the BASELINE size (N=1024, K=512, L=8,
  2^16+ frames): noiseless codewords decode to their messages, results do not
  depend on batch composition or grid size.
All calls go through the C-ABI (libqpd.so); nothing here falls back to a CPU
decoder.
"""
import os

import numpy as np
import pytest

from conftest import assert_engine, assert_frames_equal, golden_files, golden_packed, load_golden

pytestmark = pytest.mark.gpu

KINDS = ["SC-LUT", "SCL-LUT", "FastSC-LUT", "FastSCL-LUT"]


@pytest.fixture(scope="module")
def qpd(native_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import quantized_decoder_polar_codes_amd as Q

    return Q


def _node_type(N, K):
    from quantized_decoder_polar_codes_amd import codes as C

    _, mb, fm, mm = C.construct_pw(N, K)
    return fm, C.identify_nodes(N, mb).astype(np.int32)


ENGINES = ["auto", "generic"]  # auto = the fast kernel wherever the tables allow it


def fast_engine_serves(kind, L):
    """The fast engine takes L <= 8, and SCL-LUT (CA-SCL-LUT) up to L = 16 (lane groups of 16,
    qpd_fast_select.hpp select_survivors16); larger lists run on the generic engine."""
    if "SCL" not in kind:  # SC-LUT / FastSC-LUT: no list
        return True
    return L <= 8 or (L <= 16 and kind in ("SCL-LUT", "CA-SCL-LUT"))


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("path", golden_files(), ids=lambda p: os.path.basename(p)[:-4])
def test_gpu_matches_golden(path, engine, qpd):
    g = load_golden(path)
    N, K, L = int(g["N"]), int(g["K"]), int(g["L"])
    if str(g["kind"]) == "SC":
        if engine != "auto":
            pytest.skip("float SC has one kernel")
        dec = qpd.SCDecoder(N, K, g["frozen"], 1 - g["frozen"])
        got = dec.decode_batch(g["llr"])
    else:
        kw = {"A": int(g["A"])} if str(g["kind"]).startswith("CA-") else {}
        dec = qpd.from_packed(str(g["kind"]), golden_packed(g), K, g["frozen"], L=L, node_type=g["node_type"],
                              engine=engine, **kw)
        assert dec.info()["engine"] == (2 if engine == "auto" and fast_engine_serves(str(g["kind"]), L) else 1)
        got = dec.decode_batch(g["symbols"].astype(np.int32))
    assert_frames_equal(got, g["expected"], dec, f"golden-{os.path.basename(path)[:-4]}-{engine}")


CASES = [
    # N, K, L, table kind
    (2, 1, 2, "random"),
    (4, 2, 2, "random"),
    (8, 4, 3, "random"),
    (16, 8, 4, "random"),
    (32, 16, 8, "perelem"),
    (64, 20, 5, "random"),
    (128, 32, 8, "random"),
    (128, 64, 8, "continuous"),
    (256, 128, 7, "random"),
    (512, 256, 8, "minsum"),
    (1024, 512, 8, "random"),
    (1024, 512, 1, "random"),
    # L > 8: 2L > 16 candidates, libstdc++ introsort replayed per selection
    (32, 16, 9, "random"),
    (64, 32, 16, "random"),
    (128, 64, 16, "minsum"),
    (128, 80, 21, "random"),
    (256, 128, 32, "random"),
    (512, 256, 16, "perelem"),
]


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("N,K,L,tables", CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_gpu_matches_oracle(N, K, L, tables, kind, engine, qpd, oracle_mod):
    from quantized_decoder_polar_codes_amd import lut as LU

    seed = 1000 + N + 7 * L + KINDS.index(kind)
    if tables == "minsum":
        p = LU.minsum_uniform_luts(N)
    elif tables == "continuous":
        p = LU.random_luts(N, 16, seed=seed, distinct_mags=None)
    else:
        p = LU.random_luts(N, 16, seed=seed, distinct_mags=3, per_element=(tables == "perelem"))
    fm, nt = _node_type(N, K)
    B = 24 if N >= 1024 and kind in ("SCL-LUT", "FastSCL-LUT") else 200
    sym = np.random.default_rng(seed).integers(0, 16, size=(B, N), dtype=np.int32)
    special_root = (kind == "FastSC-LUT" and 0 <= nt[0] <= 3) or (kind == "FastSCL-LUT" and 0 <= nt[0] <= 2)
    if special_root:  # undefined behaviour in the reference: both sides refuse
        with pytest.raises(RuntimeError):
            oracle_mod.decode_lut(kind, p, K, L, fm, sym, node_type=nt)
        with pytest.raises(ValueError):
            qpd.from_packed(kind, p, K, fm, L=L, node_type=nt, engine=engine)
        return
    want = oracle_mod.decode_lut(kind, p, K, L, fm, sym, node_type=nt)
    dec = qpd.from_packed(kind, p, K, fm, L=L, node_type=nt, engine=engine)
    if engine == "auto":
        assert dec.info()["engine"] == (2 if tables != "perelem" and fast_engine_serves(kind, L) else 1)
    got = dec.decode_batch(sym)
    redo = lambda rows: qpd.from_packed(kind, p, K, fm, L=L, node_type=nt, engine=engine).decode_batch(sym[rows])  # noqa: E731
    assert_frames_equal(got, want, dec, f"oracle-{kind}-{N}-{K}-{L}-{tables}-{engine}", redo, sym)


CA_CASES = [
    # N, A, crc_n, L, tables, Eb/N0
    (32, 6, 24, 2, "minsum", 3.0),
    (64, 20, 24, 4, "minsum", 2.0),
    (128, 40, 24, 8, "minsum", 1.0),
    (128, 40, 24, 8, "random", 1.0),
    (128, 40, 24, 16, "random", 1.0),  # L = 16: SCL on the fast engine's lane groups of 16
    (256, 100, 24, 12, "minsum", 1.0),
    (256, 100, 11, 8, "minsum", 1.5),   # a shorter CRC (5G CRC11 taps)
    (512, 230, 24, 3, "minsum", 1.5),
    (1024, 488, 24, 8, "minsum", 1.5),
    (1024, 500, 24, 8, "minsum", 1.5),  # K - A = 12 < crc_n: only the first 12 check bits compared
]
CRC11_LOC = (11, 10, 9, 5, 0)


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("N,A,crc_n,L,tables,ebn0", CA_CASES)
@pytest.mark.parametrize("kind", ["CA-SCL-LUT", "CA-FastSCL-LUT"])
def test_gpu_ca_matches_oracle(N, A, crc_n, L, tables, ebn0, kind, engine, qpd, oracle_mod):
    """CRC-aided decoders on frames that carry a real CRC, so the CRC decides
    the output path on many frames (checked below)."""
    from quantized_decoder_polar_codes_amd import codes as C
    from quantized_decoder_polar_codes_amd import lut as LU

    loc = oracle_mod.CRC24_LOC if crc_n == 24 else CRC11_LOC
    K = 512 if (N, A) == (1024, 500) else A + crc_n
    seed = 5000 + N + A + L
    _, mb, fm, mm = C.construct_pw(N, K)
    nt = C.identify_nodes(N, mb).astype(np.int32)
    p = LU.minsum_uniform_luts(N) if tables == "minsum" else LU.random_luts(N, 16, seed=seed, distinct_mags=3)
    rng = np.random.default_rng(seed)
    B = 48 if N >= 1024 else 300
    msg = rng.integers(0, 2, size=(B, A), dtype=np.uint8)
    u = np.concatenate([msg, oracle_mod.crc_encode(msg, crc_n, loc)[:, : K - A]], axis=1)
    x = C.polar_encode(u, mb, N)
    sigma = np.sqrt(1 / (2 * (K / N) * 10 ** (ebn0 / 10)))
    llr = ((1.0 - 2.0 * x) + rng.normal(0, sigma, size=(B, N))) * 2 / sigma ** 2
    sym = np.clip(np.rint(llr / 0.5 + 7.5), 0, 15).astype(np.int32)
    special_root = kind == "CA-FastSCL-LUT" and 0 <= nt[0] <= 2
    if special_root:
        with pytest.raises(ValueError):
            qpd.from_packed(kind, p, K, fm, L=L, node_type=nt, engine=engine, A=A, crc_n=crc_n, crc_loc=loc)
        return
    want = oracle_mod.decode_lut_ca(kind, p, K, A, L, fm, sym, node_type=nt, crc_n=crc_n, crc_loc=loc)
    dec = qpd.from_packed(kind, p, K, fm, L=L, node_type=nt, engine=engine, A=A, crc_n=crc_n, crc_loc=loc)
    assert dec.info()["out_bits"] == A
    got = dec.decode_batch(sym)
    assert got.shape == (B, A)
    redo = lambda rows: qpd.from_packed(kind, p, K, fm, L=L, node_type=nt, engine=engine, A=A, crc_n=crc_n,  # noqa: E731
                                        crc_loc=loc).decode_batch(sym[rows])
    assert_frames_equal(got, want, dec, f"ca-{kind}-{N}-{A}-{crc_n}-{L}-{tables}-{engine}", redo, sym)


def test_ca_dropin_api(qpd, oracle_mod):
    """The reference's constructor order / kwargs and one-frame decode()."""
    from PolarDecoder.Decoder.CAFastSCLLUTDecoder import CAFastSCLLUTDecoder
    from PolarDecoder.Decoder.CASCLLUTDecoder import CASCLLUTDecoder
    from quantized_decoder_polar_codes_amd import codes as C
    from quantized_decoder_polar_codes_amd import lut as LU

    N, A, L = 128, 40, 8
    K = A + 24
    _, mb, fm, mm = C.construct_pw(N, K)
    nt = C.identify_nodes(N, mb).astype(np.int32)
    p = LU.minsum_uniform_luts(N)
    fs, gs, vcl = LU.unpack_to_reference(p)
    sym = np.random.default_rng(3).integers(2, 14, size=(5, N), dtype=np.int32)
    d0 = CASCLLUTDecoder(N, K, A, L, fm.tolist(), mm.tolist(), 24, list(oracle_mod.CRC24_LOC), fs, gs, vcl)
    d1 = CAFastSCLLUTDecoder(N=N, K=K, A=A, L=L, frozen_bits=fm, message_bits=mm, node_type=nt, LUT_f=fs,
                                LUT_g=gs, virtual_channel_llr=vcl)
    for d, kind in ((d0, "CA-SCL-LUT"), (d1, "CA-FastSCL-LUT")):
        want = oracle_mod.decode_lut_ca(kind, p, K, A, L, fm, sym, node_type=nt)
        for i in range(len(sym)):
            out = d.decode(sym[i][None])
            assert out.dtype == np.uint8 and out.shape == (A,)
            assert np.array_equal(out, want[i])


def test_sc_float_matches_oracle(qpd, oracle_mod):
    from quantized_decoder_polar_codes_amd import codes as C

    for N, K in [(2, 1), (16, 8), (128, 32), (1024, 512)]:
        _, _, fm, mm = C.construct_pw(N, K)
        rng = np.random.default_rng(N)
        llr = rng.normal(0.5, 3, size=(300, N))
        llr[::5, ::3] = 0.0
        want = oracle_mod.decode_sc_float(N, K, fm, llr)
        got = qpd.SCDecoder(N, K, fm, mm).decode_batch(llr)
        assert (got == want).all(), N


def test_dropin_nested_list_api(qpd, oracle_mod):
    """The reference's constructor/decode surface, fed nested lists exactly as
    mainQuantizedDecoder_LLRDomain.py:87-102 builds them."""
    from PolarDecoder.Decoder.FastSCLLUTDecoder import FastSCLLUTDecoder
    from PolarDecoder.Decoder.FastSCLUTDecoder import FastSCLUTDecoder
    from PolarDecoder.Decoder.SCLLUTDecoder import SCLLUTDecoder
    from PolarDecoder.Decoder.SCLUTDecoder import SCLUTDecoder
    from quantized_decoder_polar_codes_amd import codes as C
    from quantized_decoder_polar_codes_amd import lut as LU

    N, K, L = 128, 64, 8
    p = LU.random_luts(N, 16, seed=77, distinct_mags=4)
    fs, gs, vcl = LU.unpack_to_reference(p)
    _, mb, fm, mm = C.construct_pw(N, K)
    nt = C.identify_nodes(N, mb).astype(np.int32)
    decs = {
        "SC-LUT": SCLUTDecoder(N, K, fm, mm, fs, gs, vcl),
        "SCL-LUT": SCLLUTDecoder(N, K, L, fm, mm, fs, gs, vcl),
        "FastSC-LUT": FastSCLUTDecoder(N=N, K=K, frozen_bits=fm, message_bits=mm, node_type=nt, LUT_Fs=fs,
                                       LUT_Gs=gs, virtual_channel_llr=vcl),
        "FastSCL-LUT": FastSCLLUTDecoder(N, K, L, fm, mm, nt, fs, gs, vcl),
    }
    sym = np.random.default_rng(5).integers(0, 16, size=(6, N), dtype=np.int32)
    for kind, d in decs.items():
        want = oracle_mod.decode_lut(kind, p, K, L, fm, sym, node_type=nt)
        for b in range(len(sym)):
            one = d.decode(sym[b][None].astype(np.int64))  # (1, N) int64 is force-cast like pybind11
            assert one.dtype == np.uint8 and one.shape == (K,)
            assert (one == want[b]).all(), kind


def test_torch_device_path_matches_host_path(qpd):
    import torch

    from quantized_decoder_polar_codes_amd import lut as LU

    N, K, L = 1024, 512, 8
    p = LU.minsum_uniform_luts(N)
    fm, nt = _node_type(N, K)
    d = qpd.from_packed("SCL-LUT", p, K, fm, L=L)
    sym = np.random.default_rng(9).integers(0, 16, size=(300, N), dtype=np.int32)
    host = d.decode_batch(sym)
    dev = d.decode_batch(torch.from_numpy(sym).cuda())
    torch.cuda.synchronize()
    assert dev.is_cuda and dev.dtype == torch.uint8
    assert (dev.cpu().numpy() == host).all()


@pytest.mark.parametrize("engine", ["gpu", pytest.param("host", marks=pytest.mark.host_engine)])
def test_out_of_range_symbol_is_reported(engine, qpd):
    from quantized_decoder_polar_codes_amd import lut as LU

    N, K = 64, 32
    p = LU.random_luts(N, 16, seed=1)
    fm, nt = _node_type(N, K)
    d = qpd.from_packed("SC-LUT", p, K, fm)
    d.set_host_engine("cpu" if engine == "host" else "gpu")
    sym = np.zeros((3, N), dtype=np.int32)
    sym[1, 7] = 16
    with pytest.raises(ValueError):
        d.decode_batch(sym)
    assert_engine(d, engine)
    d.decode_batch(np.zeros((3, N), dtype=np.int32))  # flag cleared


def _noiseless_symbols(msg, msgbits, N, v=16):
    from quantized_decoder_polar_codes_amd import codes as C

    x = C.polar_encode(msg, msgbits, N)
    return np.where(x == 0, v - 1, 0).astype(np.int32)  # strongest +/- quanta


@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("kind", KINDS)
def test_full_size_noiseless_roundtrip(kind, engine, qpd):
    """BASELINE size (N=1024, K=512, L=8): encode -> noiseless channel -> decode
    returns every message, over 2^16 frames (SCL) / 2^17 (SC)."""
    from quantized_decoder_polar_codes_amd import codes as C
    from quantized_decoder_polar_codes_amd import lut as LU

    N, K, L = 1024, 512, 8
    _, mb, fm, mm = C.construct_pw(N, K)
    nt = C.identify_nodes(N, mb).astype(np.int32)
    B = 1 << (16 if "SCL" in kind else 17)
    msg = np.random.default_rng(11).integers(0, 2, size=(B, K), dtype=np.uint8)
    sym = _noiseless_symbols(msg, mb, N)
    d = qpd.from_packed(kind, LU.minsum_uniform_luts(N), K, fm, L=L, node_type=nt, engine=engine)
    got = d.decode_batch(sym)
    assert (got == msg).all()


@pytest.mark.parametrize("engine", ENGINES)
def test_batch_and_grid_invariance(engine, qpd):
    """A frame's bits do not depend on its batch neighbours, the batch size or
    the persistent-grid size (grid-stride path)."""
    from quantized_decoder_polar_codes_amd import lut as LU

    N, K, L = 256, 128, 8
    p = LU.random_luts(N, 16, seed=21, distinct_mags=3)
    fm, nt = _node_type(N, K)
    sym = np.random.default_rng(3).integers(0, 16, size=(517, N), dtype=np.int32)
    mk = lambda **kw: qpd.from_packed("FastSCL-LUT", p, K, fm, L=L, node_type=nt, engine=engine, **kw)  # noqa: E731
    a = mk().decode_batch(sym)
    b = mk(max_waves=3).decode_batch(sym)
    c = mk().decode_batch(sym[100:107])
    assert (a == b).all()
    assert (a[100:107] == c).all()


def test_fast_engine_lds_placement_sweep(qpd, oracle_mod, monkeypatch):
    """Every split of the tree between LDS and global scratch gives the same bits."""
    from quantized_decoder_polar_codes_amd import lut as LU

    N, K, L = 256, 128, 4
    p = LU.random_luts(N, 16, seed=55, distinct_mags=3)
    fm, nt = _node_type(N, K)
    sym = np.random.default_rng(56).integers(0, 16, size=(80, N), dtype=np.int32)
    for kind in ("SCL-LUT", "FastSCL-LUT", "FastSC-LUT"):
        want = oracle_mod.decode_lut(kind, p, K, L, fm, sym, node_type=nt)
        seen = set()
        for budget in (256, 1024, 2048, 4096, 8192, 65536):
            monkeypatch.setenv("QPD_LDS_BUDGET", str(budget))
            d = qpd.from_packed(kind, p, K, fm, L=L, node_type=nt, engine="fast")
            seen.add(d.info()["lds_from_depth"])
            assert (d.decode_batch(sym) == want).all(), (kind, budget)
        assert len(seen) >= 4


@pytest.mark.parametrize("N,K,L", [(256, 128, 8), (512, 420, 5), (1024, 900, 8)])
def test_fastscl_rate1_paths(N, K, L, qpd, oracle_mod, monkeypatch):
    """FastSCL rate-1 nodes through all three argsort paths: <= 16 elements in
    registers, 17..32 in the LDS tail (default budget) or, with the tree in
    global scratch (budget 256), the slab path, and > 32 elements (a 256-element
    node at N = 1024, K = 900) -- tie-heavy tables so the introsort replay
    matters."""
    from quantized_decoder_polar_codes_amd import lut as LU

    p = LU.random_luts(N, 16, seed=N + K, distinct_mags=3)
    fm, nt = _node_type(N, K)
    sym = np.random.default_rng(N - K).integers(0, 16, size=(48, N), dtype=np.int32)
    want = oracle_mod.decode_lut("FastSCL-LUT", p, K, L, fm, sym, node_type=nt)
    for budget in (None, 256):
        if budget is None:
            monkeypatch.delenv("QPD_LDS_BUDGET", raising=False)
        else:
            monkeypatch.setenv("QPD_LDS_BUDGET", str(budget))
        d = qpd.from_packed("FastSCL-LUT", p, K, fm, L=L, node_type=nt, engine="fast")
        got = d.decode_batch(sym)
        assert_frames_equal(got, want, d, f"fscl-r1-{N}-{K}-{L}-budget{budget}", None, sym)


def test_fast_engine_rejects_per_element_tables(qpd):
    from quantized_decoder_polar_codes_amd import lut as LU

    N, K = 32, 16
    p = LU.random_luts(N, 16, seed=3, per_element=True)
    fm, nt = _node_type(N, K)
    with pytest.raises(ValueError):
        qpd.from_packed("SCL-LUT", p, K, fm, L=4, engine="fast")


@pytest.mark.parametrize("kind,L", [("SC-LUT", 1), ("SCL-LUT", 8), ("FastSC-LUT", 1), ("FastSCL-LUT", 4)])
def test_gpu_with_designed_tables_matches_oracle(kind, L, qpd, oracle_mod):
    """MinDistortion tables from lutgen.py and the drivers' channel quantizer
    (the reference's whole pipeline), GPU vs oracle; BLER well below uncoded."""
    from quantized_decoder_polar_codes_amd import codes as C
    from quantized_decoder_polar_codes_amd import lutgen as LG
    from quantized_decoder_polar_codes_amd import montecarlo as MC

    N, K = 256, 128
    d = LG.design(N, 16, 3.0)
    _, mb, fm, mm = C.construct_pw(N, K)
    nt = C.identify_nodes(N, mb).astype(np.int32)
    sigma = MC.sigma_for(2.5, K / N)
    _, _, edges, clut = LG.channel_quantizer(sigma, 128, 16)
    rng = np.random.default_rng(11)
    msg = rng.integers(0, 2, size=(400, K), dtype=np.uint8)
    x = C.polar_encode(msg, mb, N)
    llr = ((1.0 - 2.0 * x) + rng.normal(0, sigma, size=x.shape)) * 2 / sigma ** 2
    sym = C.quantize_channel(llr, edges, clut, 16)
    want = oracle_mod.decode_lut(kind, d.packed(), K, L, fm, sym, node_type=nt)
    got = qpd.from_packed(kind, d.packed(), K, fm, L=L, node_type=nt).decode_batch(sym)
    assert np.array_equal(got, want)
    assert (got != msg).any(1).mean() < 0.5


def test_kernel_timing_and_lds_probe(qpd):
    """The measurement hooks bench.py relies on: per-class launch timing
    (HIP events on the launch stream) and the on-chip peak probe."""
    import ctypes

    import torch

    from quantized_decoder_polar_codes_amd import _lib
    from quantized_decoder_polar_codes_amd import lut as LU

    N, K = 256, 128
    fm, nt = _node_type(N, K)
    dec = qpd.from_packed("SCL-LUT", LU.minsum_uniform_luts(N), K, fm, L=8)
    sym = torch.randint(0, 16, (4096, N), dtype=torch.int32, device="cuda")
    dec.profile(True)
    for _ in range(3):
        out = dec.decode_batch(sym)
    kt = dec.kernel_times()
    dec.profile(False)
    assert kt["decode"][1] == 3 and kt["decode"][0] > 0
    assert kt["pre"][1] == 3  # pre-mode at N >= 16
    assert dec.kernel_times()["decode"][1] == 0  # read and forgotten
    dec.decode_batch(sym)
    assert dec.kernel_times()["decode"][1] == 0  # not recorded while disabled
    assert torch.equal(out, dec.decode_batch(sym))
    rates = {}
    for op in (_lib.QPD_PROBE_BPERMUTE, _lib.QPD_PROBE_READ_B32, _lib.QPD_PROBE_READ_B64):
        g = ctypes.c_double()
        _lib.check(_lib.load().qpd_probe_lds(0, op, ctypes.byref(g)))
        rates[op] = g.value
    assert all(1e3 < r < 1e6 for r in rates.values())  # GB/s: between 1 TB/s and 1 PB/s
    assert rates[_lib.QPD_PROBE_READ_B64] > rates[_lib.QPD_PROBE_BPERMUTE]


@pytest.mark.parametrize("engine", ["gpu", pytest.param("host", marks=pytest.mark.host_engine)])
def test_host_decode_reports_out_of_range_symbol(engine, qpd):
    """The per-frame host path (pinned staging, one stream sync; or the host
    engine) still raises on a channel symbol outside [0, v) and recovers for
    the next call."""
    from quantized_decoder_polar_codes_amd import lut as LU

    N, K = 128, 64
    fm, nt = _node_type(N, K)
    dec = qpd.from_packed("SCL-LUT", LU.minsum_uniform_luts(N), K, fm, L=4)
    dec.set_host_engine("cpu" if engine == "host" else "gpu")
    good = np.random.default_rng(3).integers(0, 16, size=(5, N), dtype=np.int32)
    bad = good.copy()
    bad[2, 7] = 16
    with pytest.raises(ValueError, match="outside"):
        dec.decode_batch(bad)
    assert_engine(dec, engine)
    a = dec.decode_batch(good)
    b = np.stack([dec.decode(x) for x in good])
    assert_engine(dec, engine)
    assert np.array_equal(a, b)
