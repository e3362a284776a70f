"""Mask search on the kernels (qpd_decode_search, include/qpd.h): one list decode against a set of CRC
masks -- every candidate's syndrome and metric, the output path by the set compare -- on the fast
engine (the LIST instantiations of lut_fast_kernel), the generic engine (its LS twin) and, next to
them, the host engine behind the same C-ABI.

The frames are those of tests/test_search_host.py (tests/search_cases.py: three RNTIs sent, noise-only
frames, two idle RNTIs in the set; crafted collisions), which checks the host engine against plain
numpy; here all six outputs of the kernels must equal
* the host engine's (metrics as the same doubles), and
* R separate decode_batch(return_status=True, crc_mask=m_i) calls on the same device, reduced by the
  header's rule (the lowest rank any mask passes, then the lowest index),
with qpd_info asserted to report what served.  The other codes' frames are AWGN codewords under two
masks of the set (every second frame under each), so that both are hit.
"""
import ctypes

import numpy as np
import pytest

import search_cases as X
import status_cases as S
import tx_cases as T
from conftest import assert_engine

pytestmark = pytest.mark.gpu
PAD = 3
NAMES = ("out", "hit", "rank", "metric", "syn", "cmet")
CANARY = dict(out=0xDD, hit=-9, rank=-8, metric=-7.0, syn=0x6EEEEEEE, cmet=-6.0)


@pytest.fixture(scope="module")
def qpd(native_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import quantized_decoder_polar_codes_amd as Q

    return Q


@pytest.fixture(scope="module")
def blind(tmp_path_factory):
    r = X.blind_reference(T.build_harness(), str(tmp_path_factory.mktemp("blind")))
    X.check_blind_reference(r[1], r[2])
    return r


def decoder_of(c, engine):
    from quantized_decoder_polar_codes_amd import decoders as D

    fm, nt, _ = S.code_of(c)
    kw = dict(A=c.A, crc_n=c.crc_n, crc_loc=c.crc_loc)
    if c.is_float:
        return D.from_quant(c.kind, c.N, c.K, fm, L=c.L, node_type=nt, quant=S.quant_of(c), **kw)
    dec = D.from_packed(c.kind, S.tables_of(c), c.K, fm, L=c.L, node_type=nt, engine=engine, **kw)
    assert dec.info()["engine"] == {"fast": 2, "generic": 1}[engine]
    return dec


def dev_search(dec, x, rows, nB=None, pad=PAD, want=NAMES):
    """qpd_decode_search as a C caller on a resident tensor: the six outputs as numpy, nB + pad frames each,
    pre-filled with canaries; frames past nB must keep them."""
    import torch

    from quantized_decoder_polar_codes_amd import _lib

    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    ty = {torch.int32: _lib.QPD_IN_I32, torch.uint8: _lib.QPD_IN_U8, torch.float64: _lib.QPD_IN_F64}[t.dtype]
    nB = t.shape[0] if nB is None else nB
    n, L = nB + pad, int(dec.L)
    o = dict(out=torch.full((n, dec.out_bits), CANARY["out"], dtype=torch.uint8, device="cuda"),
             hit=torch.full((n,), CANARY["hit"], dtype=torch.int32, device="cuda"),
             rank=torch.full((n,), CANARY["rank"], dtype=torch.int32, device="cuda"),
             metric=torch.full((n,), CANARY["metric"], dtype=torch.float64, device="cuda"),
             syn=torch.full((n, L), CANARY["syn"], dtype=torch.int32, device="cuda"),
             cmet=torch.full((n, L), CANARY["cmet"], dtype=torch.float64, device="cuda"))
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.uint8))
    rows = rows.reshape(len(rows), -1) if rows.ndim == 2 else rows.reshape(0, 0)
    sa = _lib.QpdSearchArgs()
    sa.crc_masks = rows.ctypes.data if rows.size else None
    sa.n_masks, sa.crc_mask_bits = rows.shape
    p = lambda k: o[k].data_ptr() if k in want else None  # noqa: E731
    sa.cand_syndrome, sa.cand_metric, sa.hit_mask, sa.hit_rank, sa.metric = p("syn"), p("cmet"), p("hit"), p("rank"), p("metric")
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.load().qpd_decode_search(dec._h, ctypes.c_void_p(t.data_ptr()), ty, nB,
                                             None if p("out") is None else ctypes.c_void_p(p("out")), ctypes.byref(sa),
                                             ctypes.c_void_p(st)))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in o.items()}
    got["syn"] = got["syn"].view(np.uint32)
    for k, a in got.items():
        assert (a[nB:] == CANARY[k]).all(), f"{k}: frames past B written"
        if k not in want:
            assert (a == CANARY[k]).all(), f"{k}: written though not asked for"
    return {k: a[:nB] for k, a in got.items()}


def host_engine_search(dec, x, rows):
    """The same decoder's host engine through decode_search_batch / qpd_decode_search_host."""
    dec.set_host_engine("cpu")
    try:
        r = dec.decode_search_batch(np.asarray(x), rows)
        assert_engine(dec, "host")
    finally:
        dec.set_host_engine("gpu")
    return dict(out=r.out, hit=r.hit_mask, rank=r.hit_rank, metric=r.metric, syn=r.syndrome, cmet=r.cand_metric)


def by_status_calls(dec, x, rows, cmet):
    """R separate status decodes on the device, reduced by the header's rule -> (out, hit, rank, metric)."""
    B = len(x)
    out, hit, rank, metric = None, np.full(B, -1, np.int32), np.zeros(B, np.int32), None
    for i, m in enumerate(rows):
        sb, st = dec.decode_batch(x, return_status=True, crc_mask=m)
        assert_engine(dec, "gpu")
        ok = np.asarray(st.crc_pass)
        # the status metric is the output path's own: its rank is the first candidate with that metric that ...
        rk = np.array([int(np.flatnonzero(cmet[f] == st.metric[f])[0]) for f in range(B)], np.int32)
        if out is None:
            out, metric = sb.copy(), np.asarray(st.metric).copy()  # (no pass anywhere: every run returns the best-metric path)
        better = ok & ((hit < 0) | (rk < rank))
        out[better], metric[better], hit[better], rank[better] = sb[better], st.metric[better], i, rk[better]
    return out, hit, rank, metric


def assert_same(a, b, what, names=NAMES):
    for k in names:
        assert a[k].shape == b[k].shape and (a[k] == b[k]).all(), \
            f"{what}: {k} of {(a[k] != b[k]).reshape(len(a[k]), -1).any(1).sum()} frames differ"


def check_engine_trio(c, x, rows, engine):
    dec = decoder_of(c, engine)
    got = dev_search(dec, x, rows)
    assert_engine(dec, "gpu")
    host = host_engine_search(dec, x, rows)
    assert_same(got, host, f"{c.id} {engine} vs host engine")
    out, hit, rank, metric = by_status_calls(dec, x, rows, got["cmet"])
    # equal metrics within a frame make the rank read off the status metric ambiguous: compare it where they differ
    clear = np.array([(got["cmet"][f] == metric[f]).sum() == 1 for f in range(len(x))])
    assert (got["out"] == out).all() and (got["hit"] == hit).all() and (got["metric"] == metric).all()
    assert (got["rank"][clear] == rank[clear]).all() and clear.sum() * 2 > len(x)
    return dec, got


# -- the blind-detection frames and the crafted collisions --------------------------------------------------------

@pytest.mark.parametrize("engine", ["fast", "generic"])
def test_blind_frames_on_the_kernels(engine, qpd, blind, monkeypatch):
    for name in S.SWITCH_ENV:
        monkeypatch.delenv(name, raising=False)
    x, sent, ref, syn, cmet = blind
    rows = X.mask_rows(X.RNTI_SET, 16)
    dec, got = check_engine_trio(X.BLIND, x, rows, engine)
    w_out, w_hit, w_rank, w_met = ref
    assert (got["out"] == w_out).all() and (got["hit"] == w_hit).all() and (got["rank"] == w_rank).all()
    assert (got["metric"] == w_met).all() and (got["syn"] == syn).all() and (got["cmet"] == cmet).all()
    # crafted collisions: masks [S[f0][3], S[f0][1]] -> rank 1, index 1; duplicates -> the first index
    f0 = next(f for f in range(len(x)) if len(set(syn[f, :4].tolist())) == 4 and np.isfinite(cmet[f, :4]).all())
    g = dev_search(dec, x, X.mask_rows([syn[f0, 3], syn[f0, 1]], 24))
    assert g["rank"][f0] == 1 and g["hit"][f0] == 1 and g["metric"][f0] == cmet[f0, 1]
    g = dev_search(dec, x, X.mask_rows([syn[f0, 3], syn[f0, 2], syn[f0, 2], syn[f0, 3]], 24))
    assert g["rank"][f0] == 2 and g["hit"][f0] == 1
    # n_masks = 0: the syndromes and metrics of a call with masks, nothing else
    g0 = dev_search(dec, x, [], want=("syn", "cmet"))
    assert_same(g0, got, "n_masks = 0", ("syn", "cmet"))
    # R = 256, the planted mask last: the whole set is walked
    rng = np.random.default_rng(5)
    big = rng.integers(0, 2, size=(256, 24), dtype=np.uint8)
    big[255] = X.mask_rows([syn[f0, 2]], 24)[0]
    g = dev_search(dec, x, big)
    hit, rank = X.search_from_syndromes(syn, [X.mask_value(r) for r in big], 0)
    assert (g["hit"] == hit).all() and (g["rank"] == rank).all() and g["hit"][f0] == 255 and g["rank"][f0] == 2


# -- input types, batch sizes, the Python call ---------------------------------------------------------------------

@pytest.mark.parametrize("nB", [1, 37, 4096])
def test_input_types_and_batch_sizes(nB, qpd, blind, monkeypatch):
    import torch

    for name in S.SWITCH_ENV:
        monkeypatch.delenv(name, raising=False)
    x = np.resize(blind[0], (nB, X.BLIND.N))
    rows = X.mask_rows(X.RNTI_SET, 16)
    dec = decoder_of(X.BLIND, "fast")
    want = host_engine_search(dec, x, rows)
    got = dev_search(dec, x, rows, nB=nB)
    assert_engine(dec, "gpu")
    assert_same(got, want, f"int32, B = {nB}")
    t8 = torch.from_numpy(x.astype(np.uint8)).cuda()
    assert_same(dev_search(dec, t8, rows, nB=nB), want, f"uint8, B = {nB}")
    # more frames in the buffer than the call decodes: the rest keep their canaries (dev_search)
    if nB == 37:
        full = np.resize(blind[0], (40, X.BLIND.N))
        assert_same(dev_search(dec, full, rows, nB=37, pad=3), want, "B = 37 of 40")
    # the Python call: resident tensors in, tensors out; numpy in, numpy out
    r = dec.decode_search_batch(t8, list(X.RNTI_SET))
    assert_engine(dec, "gpu")
    assert r.out.is_cuda and r.hit_mask.dtype == torch.int32 and r.syndrome.dtype == torch.uint32 and r.cand_metric.dtype == torch.float64
    py = dict(out=r.out, hit=r.hit_mask, rank=r.hit_rank, metric=r.metric, syn=r.syndrome.view(torch.int32), cmet=r.cand_metric)
    py = {k: v.cpu().numpy() for k, v in py.items()}
    py["syn"] = py["syn"].view(np.uint32)
    assert_same(py, want, "CUDA tensor through decode_search_batch")
    n = dec.decode_search_batch(x, rows)  # (QPD_HOST_ENGINE=gpu: the GPU behind the host call)
    assert_engine(dec, "gpu")
    assert isinstance(n.out, np.ndarray) and n.syndrome.dtype == np.uint32
    assert_same(dict(out=n.out, hit=n.hit_mask, rank=n.hit_rank, metric=n.metric, syn=n.syndrome, cmet=n.cand_metric), want, "numpy")
    e = dec.decode_search_batch(t8, [])
    assert e.out is None and e.hit_mask is None and (e.syndrome.view(torch.int32).cpu().numpy().view(np.uint32) == want["syn"]).all()
    if nB == 1:
        with pytest.raises(ValueError):
            dec.decode_search_batch(x, np.full((2, 16), 2, np.uint8))


# -- the instantiations ----------------------------------------------------------------------------------------------

def masked_frames(c, vals, bits):
    """Quantized AWGN observations of codewords whose CRC carries vals[f % len(vals)] (a `bits`-bit mask), around
    the case's Eb/N0 as tests/status_cases.py draws its CRC frames."""
    import oracle
    from quantized_decoder_polar_codes_amd import codes as C

    rng = np.random.default_rng(S.seed_of(c))
    _, _, mb = S.code_of(c)
    msg = rng.integers(0, 2, size=(c.B, c.A), dtype=np.uint8)
    chk = oracle.crc_encode(msg, c.crc_n, c.crc_loc)
    for f in range(c.B):
        chk[f] ^= T.placed_mask(X.mask_rows([vals[f % len(vals)]], bits)[0], c.crc_n)
    info = np.concatenate([msg, chk[:, : c.K - c.A], np.zeros((c.B, c.K - c.A - min(c.crc_n, c.K - c.A)), np.uint8)], axis=1)
    cw = C.polar_encode(info, mb, c.N)
    ebn0 = c.ebn0 + np.linspace(-1.5, 1.5, c.B)[:, None]
    sigma = np.sqrt(1 / (2 * (c.K / c.N) * 10 ** (ebn0 / 10)))
    llr = ((1.0 - 2.0 * cw) + rng.normal(0, sigma, size=cw.shape)) * 2 / sigma ** 2
    if c.is_float:
        return llr
    return np.clip(np.rint(llr / 0.5 + 7.5), 0, 15).astype(np.int32)


def _c(kind, N, K, L, A, engine="fast", B=203, ebn0=1.0, tables="minsum", crc_n=24):
    return S.Case(kind, N, K, L, tables, engine=engine, A=A, crc_n=crc_n, ebn0=ebn0, B=B)


INST = [
    _c("CA-SCL-LUT", 128, 64, 2, 40),
    _c("CA-SCL-LUT", 128, 64, 4, 40),
    _c("CA-SCL-LUT", 128, 64, 8, 40),
    _c("CA-SCL-LUT", 128, 64, 12, 40),   # W16
    _c("CA-SCL-LUT", 128, 64, 16, 40),   # W16
    _c("CA-SCL-LUT", 128, 64, 4, 56),    # chk = 8 < crc_n
    _c("CA-FastSCL-LUT", 128, 64, 8, 40),
    _c("CA-FastSCL-LUT", 128, 64, 16, 40),  # engine="fast": lane groups of 16
    _c("CA-SCL-LUT", 128, 64, 8, 40, engine="generic"),
    _c("CA-SCL", 64, 32, 4, 8, engine="generic", tables="awgn", B=64),
    _c("CA-SCL-LUT", 1024, 512, 8, 488, B=256, ebn0=2.0),  # full size: prefix stages, split tail in the plain kernel
]
# 24-bit masks that differ in their top 8 bits too (the short compare sees those alone; there the first and
# the third coincide); the frames carry the second and the fourth
SET_VALS = (0x00A500, 0x3C3C00, 0x000100, 0x800100)


def inst_inputs(c):
    return masked_frames(c, (SET_VALS[1], SET_VALS[3]), 24), X.mask_rows(SET_VALS, 24)


# QPD_SETS (frame sets per wave) is the fast engine's: its cases run at 1 and 2, the generic engine's once
INST_SETS = [(c, s) for c in INST for s in (("1", "2") if c.engine == "fast" else ("1",))]


@pytest.mark.parametrize("c,sets", INST_SETS, ids=lambda v: v.id if isinstance(v, S.Case) else f"sets{v}")
def test_instantiations(c, sets, qpd, monkeypatch):
    for name in S.SWITCH_ENV:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("QPD_SETS", sets)
    assert not S.special_root(c)
    x, rows = inst_inputs(c)
    dec, got = check_engine_trio(c, x, rows, c.engine)
    info = dec.info()
    assert info["engine"] == (1 if c.engine == "generic" else 2) and info["last_engine"] == 1
    if c.engine == "fast":
        assert info["lanes_per_frame"] == (16 if c.L > 8 else c.L)
    if c.N == 1024:
        assert info["prefix_ops"] > 0
        sb, st = dec.decode_batch(x, return_status=True, crc_mask=rows[1])
        one = dev_search(dec, x, rows[1:2])
        assert (one["out"] == sb).all() and (one["metric"] == st.metric).all() and ((one["hit"] >= 0) == st.crc_pass).all()
    # not vacuous: both sent masks are hit, some frames are not, and where chk covers the mask a hit is not always rank 0
    assert {1, 3} <= set(got["hit"].tolist()) and (got["hit"] < 0).any()
    if c.nchk >= 16 and c.L >= 4 and c.N <= 128:
        assert (got["rank"] > 0).any()
