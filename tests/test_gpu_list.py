"""List output on the kernels (qpd_decode_list, include/qpd.h): every path of the list in
the reference's argsort order with its K decisions, metric and CRC verdict, on the fast
engine (the LIST instantiations of lut_fast_kernel), the generic engine (its LS twin) and,
next to them, the host engine behind the same C-ABI.

Inputs are codewords over AWGN at about 1 dB (a spread of +-1.5 dB, as tests/status_cases.py
draws its CRC frames) on the tie-heavy tables of the status sweep.  Every case first asserts
on the CPU oracle alone that its frames are not vacuous (check_inputs), then:

* LUT kinds: fast = generic = host engine, bit for bit on bits, metrics, flags, chosen and out;
* the oracle's status (all metrics, the winner's rank, the bits) on every engine;
* SCL-LUT / CA-SCL-LUT at L <= 8 against tests/list_ref.py;
* CRC-aided kinds: for each candidate j of a few frames, the mask under which j's compare
  succeeds, handed to the already-pinned decode_batch(return_status=True): it must pass and
  return the first candidate, in list order, whose tail matches under that mask;
* out = decode_batch's bits, metric[chosen] = the status metric; frames past B untouched.
The float kinds: against the host engine where it decodes them, else the oracle's status.
"""
import ctypes

import numpy as np
import pytest

import list_ref
import status_cases as S
import status_ref
from conftest import assert_engine
from test_list_host import check_against_oracle

pytestmark = pytest.mark.gpu
PAD = 3  # canary frames after frame B
B = 203  # no multiple of any frames-per-wave count


@pytest.fixture(scope="module")
def qpd(native_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import quantized_decoder_polar_codes_amd as Q

    return Q


def _c(kind, N, K, L, tables="minsum", A=0, seed=0, **kw):
    return S.Case(kind, N, K, L, tables, A=A, crc_n=24 if A else 0, ebn0=1.0, B=B, seed=seed, **kw)


# the smallest shapes that reach each branch of the tail: N = 16 (one masked word), K = 30 (byte stores),
# K = 32 (dword stores), N = 256 at L = 8 and N = 512 at L = 16 (the plain tail would split), lane groups
# of 2 .. 16, FastSCL-LUT with R0 / R1 / REP nodes at L = 8 and L = 16
LUT_CASES = [
    _c("SCL-LUT", 16, 10, 4),
    _c("SCL-LUT", 64, 30, 2),
    _c("SCL-LUT", 64, 32, 8),
    _c("SCL-LUT", 64, 32, 12, "random"),
    _c("SCL-LUT", 256, 128, 8),
    _c("SCL-LUT", 512, 256, 16),
    _c("CA-SCL-LUT", 64, 40, 4, A=16),
    _c("CA-SCL-LUT", 64, 40, 8, A=16),
    _c("CA-SCL-LUT", 64, 38, 16, A=16),
    _c("CA-SCL-LUT", 256, 128, 8, A=104),
    _c("FastSCL-LUT", 128, 64, 8),
    _c("FastSCL-LUT", 128, 64, 16),
    _c("CA-FastSCL-LUT", 128, 64, 8, A=40),
    _c("CA-FastSCL-LUT", 128, 64, 12, A=40),
]


def frames_of(c):
    """Quantized AWGN observations of random codewords (with the CRC where the kind has one)."""
    from quantized_decoder_polar_codes_amd import codes as C

    rng = np.random.default_rng(S.seed_of(c))
    if c.A:
        llr = S.crc_frames(c, rng)
    else:
        _, _, mb = S.code_of(c)
        x = C.polar_encode(rng.integers(0, 2, size=(c.B, c.K), dtype=np.uint8), mb, c.N)
        ebn0 = c.ebn0 + np.linspace(-1.5, 1.5, c.B)[:, None]
        sigma = np.sqrt(1 / (2 * (c.K / c.N) * 10 ** (ebn0 / 10)))
        llr = ((1.0 - 2.0 * x) + rng.normal(0, sigma, size=x.shape)) * 2 / sigma ** 2
    return np.clip(np.rint(llr / 0.5 + 7.5), 0, 15).astype(np.int32)


_REF = {}


def oracle_status(c, mask=None):
    """(frames, (bits, pml, winner, passed)) of the CPU oracle; computed once per case, not to be written to."""
    import oracle

    key = (c.ref_key(), None if mask is None else tuple(mask))
    if key not in _REF:
        fm, nt, _ = S.code_of(c)
        x = frames_of(c)
        kw = dict(A=c.A, crc_n=c.crc_n, crc_loc=c.crc_loc, mask=mask) if c.A else {}
        _REF[key] = x, oracle.decode_lut_status(c.kind, S.tables_of(c), c.K, c.L, fm, x, node_type=nt, **kw)
    return _REF[key]


def rank_of_winner(pml, w):
    pw = pml[np.arange(len(w)), w][:, None]
    return ((pml < pw) | ((pml == pw) & (np.arange(pml.shape[1])[None] < w[:, None]))).sum(1)


def check_inputs(c, ref):
    """Not vacuous, on the oracle alone: lists of several live paths, exact metric ties, and for the
    CRC-aided kinds frames decided by a candidate other than 0 and frames no candidate passes."""
    bits, pml, winner, passed = ref
    finite = np.isfinite(pml)
    assert (finite.sum(1) >= 2).sum() * 2 >= len(pml), f"{c.id}: lists of one live path"
    srt = np.sort(np.where(finite, pml, np.nan), axis=1)
    assert (np.diff(srt, axis=1) == 0).any(), f"{c.id}: no exact tie among the finite metrics"
    if c.A:
        assert (passed & (rank_of_winner(pml, winner) != 0)).any(), f"{c.id}: chosen is always 0"
        assert (~passed).any(), f"{c.id}: every frame passes"


def decoder_of(c, engine):
    from quantized_decoder_polar_codes_amd import decoders as D

    fm, nt, _ = S.code_of(c)
    kw = dict(A=c.A, crc_n=c.crc_n, crc_loc=c.crc_loc) if c.A else {}
    if c.is_float:
        return D.from_quant(c.kind, c.N, c.K, fm, L=c.L, node_type=nt, quant=S.quant_of(c), **kw)
    dec = D.from_packed(c.kind, S.tables_of(c), c.K, fm, L=c.L, node_type=nt, engine=engine, **kw)
    assert dec.info()["engine"] == {"fast": 2, "generic": 1}[engine]
    return dec


def dev_list(dec, x, mask=None, nB=None, pad=PAD, crc_pass=True):
    """qpd_decode_list as a C caller: (bits, metric, pass, chosen, out) as numpy, nB + pad frames each,
    pre-filled with canaries (bits 0xEE, metric -7, pass 0x55, chosen -3, out 0xDD)."""
    import torch

    from quantized_decoder_polar_codes_amd import _lib

    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    ty = {torch.int32: _lib.QPD_IN_I32, torch.uint8: _lib.QPD_IN_U8, torch.float64: _lib.QPD_IN_F64}[t.dtype]
    nB = t.shape[0] if nB is None else nB
    n, L, K = nB + pad, int(dec.L), int(dec.K)
    out = torch.full((n, dec.out_bits), 0xDD, dtype=torch.uint8, device="cuda")
    b = torch.full((n, L, K), 0xEE, dtype=torch.uint8, device="cuda")
    m = torch.full((n, L), -7.0, dtype=torch.float64, device="cuda")
    ok = torch.full((n, L), 0x55, dtype=torch.uint8, device="cuda")
    ch = torch.full((n,), -3, dtype=torch.int32, device="cuda")
    la = _lib.QpdListArgs()
    if mask is not None:
        mask = np.ascontiguousarray(mask, dtype=np.uint8)
        la.crc_mask, la.crc_mask_bits = mask.ctypes.data, len(mask)
    la.cand_bits, la.cand_metric, la.chosen = b.data_ptr(), m.data_ptr(), ch.data_ptr()
    if crc_pass:
        la.cand_pass = ok.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.load().qpd_decode_list(dec._h, ctypes.c_void_p(t.data_ptr()), ty, nB, ctypes.c_void_p(out.data_ptr()),
                                           ctypes.byref(la), ctypes.c_void_p(st)))
    torch.cuda.synchronize()
    got = tuple(a.cpu().numpy() for a in (b, m, ok, ch, out))
    for a, canary in zip(got, (0xEE, -7.0, 0x55, -3, 0xDD)):
        assert (a[nB:] == canary).all(), "frames past B written"
    return tuple(a[:nB] for a in got)


def host_engine_list(dec, x, mask=None):
    """The same decoder's host engine through decode_list_batch / qpd_decode_list_host."""
    dec.set_host_engine("cpu")
    try:
        r = dec.decode_list_batch(np.asarray(x), crc_mask=mask)
        assert_engine(dec, "host")
    finally:
        dec.set_host_engine("gpu")
    ok = np.full(r.metric.shape, 0x55, dtype=np.uint8) if r.crc_pass is None else r.crc_pass.astype(np.uint8)
    return r.bits, r.metric, ok, r.chosen, r.out


NAMES = ("bits", "metric", "pass", "chosen", "out")


def assert_same(a, b, what):
    for u, v, name in zip(a, b, NAMES):
        assert u.shape == v.shape and (u == v).all(), f"{what}: {name} of {(u != v).reshape(len(u), -1).any(1).sum()} frames differ"


def mask_cross_check(c, dec, x, got, frames):
    """Per candidate j of the frames: the mask under which j's compare succeeds, through the status call."""
    bits, metric, ok, chosen, out = got
    nchk = c.K - c.A
    for f in frames:
        cc = np.stack([status_ref.crc_check_code(bits[f, j, : c.A], c.crc_n, c.crc_loc) for j in range(c.L)])
        for j in range(c.L):
            mask = np.zeros(c.crc_n, dtype=np.uint8)
            mask[:nchk] = cc[j, :nchk] ^ bits[f, j, c.A: c.K]
            match = ((cc[:, :nchk] ^ mask[None, :nchk]) == bits[f, :, c.A: c.K]).all(1)
            assert match[j]
            first = int(np.argmax(match))
            sb, st = dec.decode_batch(x[f: f + 1], return_status=True, crc_mask=mask)
            assert bool(st.crc_pass[0]), (f, j)
            assert (sb[0] == bits[f, first, : c.A]).all(), (f, j, first)
            assert st.metric[0] == metric[f, first], (f, j, first)


@pytest.mark.parametrize("sets", ["1", "2"])
@pytest.mark.parametrize("c", LUT_CASES, ids=lambda c: c.id)
def test_lut_list_on_every_engine(c, sets, qpd, monkeypatch):
    for name in S.SWITCH_ENV:
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("QPD_SETS", sets)
    assert not S.special_root(c)
    mask = S.crc_mask(16) if c.A else None
    for mk in ((None, mask) if c.A else (None,)):
        x, ref = oracle_status(c, mk)
        if mk is None:
            check_inputs(c, ref)
        fast = decoder_of(c, "fast")
        assert B % fast.info()["frames_per_wave"] != 0
        got = dev_list(fast, x, mask=mk, crc_pass=bool(c.A))
        assert_engine(fast, "gpu")
        bits, metric, ok, chosen, out = got
        check_against_oracle(c, ref, bits, metric, ok.astype(bool) if c.A else ok, chosen, out)
        # distinct candidates: the finite-metric paths of a frame differ in their bits
        fin = np.isfinite(metric)
        two = (fin.sum(1) >= 2)
        assert ((bits[two, 0] != bits[two, 1]).any(1)).all()
        if sets == "1":  # the other engines do not depend on the fast engine's frame sets
            gen = decoder_of(c, "generic")
            assert_same(got, dev_list(gen, x, mask=mk, crc_pass=bool(c.A)), "fast vs generic")
            assert_engine(gen, "gpu")
            assert_same(got, host_engine_list(gen, x, mk), "fast vs host engine")
            if c.kind in ("SCL-LUT", "CA-SCL-LUT") and c.L <= 8:
                nf = 48 if c.N <= 64 else 12
                fm, _, _ = S.code_of(c)
                wb, wm, wp, wc = list_ref.decode(S.tables_of(c), fm, c.L, x[:nf], A=c.A or None, mask=mk)
                assert (bits[:nf] == wb).all() and (metric[:nf] == wm).all() and (chosen[:nf] == wc).all()
                if c.A:
                    assert (ok[:nf] == wp).all()
        # the status call and the plain call of the same decoder
        sb, st = fast.decode_batch(x, return_status=True, crc_mask=mk)
        assert (out == sb).all() and (metric[np.arange(B), chosen] == st.metric).all()
        if c.A:
            assert (ok.astype(bool).any(1) == st.crc_pass).all()
        if mk is None:
            assert (out == fast.decode_batch(x)).all()
            if c.A:
                late = np.flatnonzero(chosen != 0)[:2].tolist()
                fail = np.flatnonzero(~ok.astype(bool).any(1))[:2].tolist()
                mask_cross_check(c, fast, x, got, sorted(set([0, 1] + late + fail)))


def test_uint8_input_python_call_and_optional_outputs(qpd, monkeypatch):
    import torch

    c = LUT_CASES[7]
    assert c.kind == "CA-SCL-LUT"
    x, _ = oracle_status(c)
    dec = decoder_of(c, "fast")
    want = dev_list(dec, x)
    r = dec.decode_list_batch(torch.from_numpy(x.astype(np.uint8)).cuda())
    assert_engine(dec, "gpu")
    assert r.bits.is_cuda and r.metric.dtype == torch.float64 and r.crc_pass.dtype == torch.bool and r.chosen.dtype == torch.int32
    got = (r.bits, r.metric, r.crc_pass.to(torch.uint8), r.chosen, r.out)
    assert_same(tuple(a.cpu().numpy() for a in got), want, "uint8 CUDA tensor")
    # numpy in (the GPU behind the host call, QPD_HOST_ENGINE=gpu), numpy out
    n = dec.decode_list_batch(x)
    assert_engine(dec, "gpu")
    assert isinstance(n.bits, np.ndarray)
    assert_same((n.bits, n.metric, n.crc_pass.astype(np.uint8), n.chosen, n.out), want, "numpy")
    # without d_out and without the optional outputs: the same candidates
    from quantized_decoder_polar_codes_amd import _lib

    t = torch.from_numpy(x).cuda()
    b = torch.full((B, c.L, c.K), 0xEE, dtype=torch.uint8, device="cuda")
    la = _lib.QpdListArgs()
    la.cand_bits = b.data_ptr()
    _lib.check(_lib.load().qpd_decode_list(dec._h, ctypes.c_void_p(t.data_ptr()), _lib.QPD_IN_I32, B, None, ctypes.byref(la),
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert (b.cpu().numpy() == want[0]).all()
    # refusals reach the caller as ValueError before any launch
    scl = decoder_of(LUT_CASES[2], "fast")
    with pytest.raises(ValueError):
        scl.decode_list_batch(x[:, :64], crc_mask=S.crc_mask(16))


FLOAT_CASES = [
    S.Case("SCL", 64, 32, 4, "ties", B=64),
    S.Case("SCL", 64, 32, 12, "ties", B=64),
    S.Case("FastSCL", 128, 64, 8, "ties", B=64),
    S.Case("CA-SCL", 64, 32, 8, "ties", A=21, crc_n=11, ebn0=1.0, B=64),
    S.Case("CA-SCL", 64, 32, 16, "awgn", A=21, crc_n=11, ebn0=1.0, B=64),
    S.Case("SCL-Uniform", 64, 32, 4, "awgn", B=64),
    S.Case("SCL-Lloyd", 64, 32, 8, "awgn", B=64),
]


@pytest.mark.parametrize("c", FLOAT_CASES, ids=lambda c: c.id)
def test_float_list(c, qpd):
    x, ref = S.reference(c)
    dec = decoder_of(c, "generic")
    for mb, want in ref.items():
        mask = S.crc_mask(mb) if mb else None
        got = dev_list(dec, x, mask=mask, nB=c.B, crc_pass=bool(c.A))
        assert_engine(dec, "gpu")
        bits, metric, ok, chosen, out = got
        check_against_oracle(c, want, bits, metric, ok.astype(bool) if c.A else ok, chosen, out)
        if c.kind not in ("SCL-Uniform", "SCL-Lloyd"):  # the host engine decodes these
            assert_same(got, host_engine_list(dec, x, mask), "generic vs host engine")
        sb, st = dec.decode_batch(x, return_status=True, crc_mask=mask)
        assert (out == sb).all() and (metric[np.arange(c.B), chosen] == st.metric).all()
