"""BOT3's in-register symbol order (QPD_BOT3_BYTEIDX, csrc/qpd_fast_bot.hpp): the height-3 bottom subtree keeps
W3 and W2 interleaved (byte k = the table index of element k as it lies) and looks its 12 internal symbols up
by those bytes.  A wrong nibble order, a u bit on the wrong byte or the second f table missed all change
bits, so every case is compared bit-exact against the CPU oracle on the seeded random tables (tie-heavy, not
min-sum: f(a, b) != f(b, a), so no order passes by symmetry), B = 77 frames (a partial last task).

Shapes, the smallest at which each path exists:
  * N = 8: BOT3 at the root, W3 from the channel (unfolded, permuted once);
  * N = 16: the root is the folded parent (W3 interleaved by the parent's lookup);
  * N = 32, 128 at K = N / 2: folded f-side and g-side parents, the folded combines;
  * N = 128 at K = 120 and K = 6: all-information and all-frozen subtrees.
The layout knobs reach the prefix kernels' unfolded BOT3 (W3 from a row / the pre-pass row) and the one-set
kernels, whose parent lookup is the bpermute form; FastSCL-LUT runs BOTX (present order) beside BOT3."""
import numpy as np
import pytest

from conftest import assert_frames_equal

pytestmark = pytest.mark.gpu

B = 77
FAST = 2  # qpd_info.engine
ENV = ("QPD_NO_PFX", "QPD_NO_PRE", "QPD_NO_BFUSE", "QPD_LDS_BUDGET", "QPD_SETS", "QPD_PFX1B", "QPD_PRE_CHUNK",
       "QPD_NO_PW1", "QPD_NO_BC2", "QPD_NO_FF", "QPD_PFX_SETS")
SHAPES = [(8, 4), (16, 8), (32, 16), (128, 64), (128, 120), (128, 6)]
# (kind, L): every instantiation that holds a BOT3
PLAIN = [("SC-LUT", 1), ("FastSC-LUT", 1), ("SCL-LUT", 2), ("SCL-LUT", 4), ("SCL-LUT", 8), ("SCL-LUT", 16),
         ("FastSCL-LUT", 8)]


@pytest.fixture(scope="module")
def qpd(native_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import quantized_decoder_polar_codes_amd as Q

    return Q


def _set_env(monkeypatch, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


_CODES, _INPUTS, _WANT = {}, {}, {}


def _code(N, K):
    if (N, K) not in _CODES:
        from quantized_decoder_polar_codes_amd import codes as C

        _, mb, fm, _ = C.construct_pw(N, K)
        _CODES[N, K] = (fm, C.identify_nodes(N, mb).astype(np.int32))
    return _CODES[N, K]


def _inputs(N, K, v):
    """Tables and symbols of a shape: shared by every kind, list size and knob (read-only)."""
    if (N, K, v) not in _INPUTS:
        from quantized_decoder_polar_codes_amd import lut as LU

        p = LU.random_luts(N, v, seed=9000 + 16 * N + K + v, distinct_mags=3)
        sym = np.random.default_rng(N * K + v).integers(0, v, size=(B, N), dtype=np.int32)
        sym[:16] = np.clip(sym[:16] // 2 + v // 2, 0, v - 1)  # a biased part: confident runs next to random frames
        _INPUTS[N, K, v] = (p, sym)
    return _INPUTS[N, K, v]


def _want(oracle_mod, kind, N, K, L, v, A=None):
    """The oracle's bits, once per (kind, shape, L, v): every knob compares against the same array."""
    key = (kind, N, K, L, v, A)
    if key not in _WANT:
        fm, nt = _code(N, K)
        p, sym = _inputs(N, K, v)
        if A is None:
            _WANT[key] = oracle_mod.decode_lut(kind, p, K, L, fm, sym, node_type=nt)
        else:
            _WANT[key] = oracle_mod.decode_lut_ca(kind, p, K, A, L, fm, sym, node_type=nt)
    return _WANT[key]


def _special_root(kind, nt):
    return "Fast" in kind and 0 <= nt[0] <= 2  # undefined in the reference


def _check(qpd, oracle_mod, kind, N, K, L, v=16, A=None, label=""):
    fm, nt = _code(N, K)
    p, sym = _inputs(N, K, v)
    kw = {} if A is None else {"A": A}
    dec = qpd.from_packed(kind, p, K, fm, L=L, node_type=nt, **kw)
    assert dec.info()["engine"] == FAST, (label, dec.info()["engine"])
    redo = lambda rows: qpd.from_packed(kind, p, K, fm, L=L, node_type=nt, **kw).decode_batch(sym[rows])  # noqa: E731
    assert_frames_equal(dec.decode_batch(sym), _want(oracle_mod, kind, N, K, L, v, A), dec, label, redo, sym)
    return dec


def _plain_cases():
    out = []
    for N, K in SHAPES:
        nt = _code(N, K)[1]
        for kind, L in PLAIN:
            if not _special_root(kind, nt):
                out.append((kind, L, N, K))
    return out


@pytest.mark.parametrize("kind,L,N,K", _plain_cases())
def test_bot3_order_matches_oracle(kind, L, N, K, qpd, oracle_mod, monkeypatch):
    _set_env(monkeypatch, {})
    _check(qpd, oracle_mod, kind, N, K, L, label=f"bot3-{kind}-L{L}-{N}-{K}")


@pytest.mark.parametrize("N,K,A", [(128, 64, 40), (128, 120, 96), (1024, 512, 488)])
@pytest.mark.parametrize("kind", ["CA-SCL-LUT", "CA-FastSCL-LUT"])
def test_bot3_order_crc_aided(kind, N, K, A, qpd, oracle_mod, monkeypatch):
    _set_env(monkeypatch, {})
    assert not _special_root(kind, _code(N, K)[1])
    _check(qpd, oracle_mod, kind, N, K, 8, A=A, label=f"bot3-{kind}-{N}-{K}-{A}")


@pytest.mark.parametrize("N,K", [(8, 4), (16, 8), (32, 16), (128, 64)])
@pytest.mark.parametrize("kind,L", [("SC-LUT", 1), ("SCL-LUT", 8), ("SCL-LUT", 16), ("FastSCL-LUT", 8)])
def test_bot3_order_v8(kind, L, N, K, qpd, oracle_mod, monkeypatch):
    """v = 8: the symbols use three bits of each nibble, the quanta rows eight lanes."""
    _set_env(monkeypatch, {})
    assert not _special_root(kind, _code(N, K)[1])
    _check(qpd, oracle_mod, kind, N, K, L, v=8, label=f"bot3-v8-{kind}-L{L}-{N}-{K}")


KNOBS = [{"QPD_SETS": "1"}, {"QPD_SETS": "2"}, {"QPD_NO_PFX": "1"}, {"QPD_NO_PW1": "1"},
         {"QPD_SETS": "1", "QPD_NO_PFX": "1"}, {"QPD_PFX1B": "1"}]


@pytest.mark.parametrize("env", KNOBS, ids=lambda e: "+".join(f"{k[4:]}={v}" for k, v in e.items()))
@pytest.mark.parametrize("kind,L,N,K", [("SCL-LUT", 8, 16, 8), ("SCL-LUT", 8, 128, 48), ("SCL-LUT", 8, 1024, 512),
                                        ("SCL-LUT", 4, 128, 64), ("SCL-LUT", 16, 128, 64), ("SC-LUT", 1, 128, 64),
                                        ("FastSCL-LUT", 8, 128, 64), ("FastSCL-LUT", 8, 1024, 512)])
def test_bot3_order_layout_knobs(kind, L, N, K, env, qpd, oracle_mod, monkeypatch):
    """One or two frame sets per wave (the one-set kernels look the folded parent up from the table register),
    the unsplit schedule, the two-word path state, and the frozen-prefix kernels with all their stages
    ((128, 48) with stage 1b: test_gpu_prefix.py), whose BOT3 reads W3 from a row."""
    assert not _special_root(kind, _code(N, K)[1])
    _set_env(monkeypatch, env)
    _check(qpd, oracle_mod, kind, N, K, L, label=f"bot3-knob-{kind}-L{L}-{N}-{K}-{env}")


def test_bot3_order_status(qpd, oracle_mod, monkeypatch):
    """The status twins (ST) run the same BOT3: the winner's path metric is the oracle's double, the CRC flag its verdict."""
    _set_env(monkeypatch, {})
    kind, N, K, A, L = "CA-SCL-LUT", 128, 64, 40, 8
    fm, nt = _code(N, K)
    p, sym = _inputs(N, K, 16)
    bits, pml, winner, passed = oracle_mod.decode_lut_status(kind, p, K, L, fm, sym, node_type=nt, A=A)
    dec = qpd.from_packed(kind, p, K, fm, L=L, node_type=nt, A=A)
    assert dec.info()["engine"] == FAST
    got, st = dec.decode_batch(sym, return_status=True)
    assert_frames_equal(got, bits, dec, "bot3-status")
    assert (np.asarray(st.metric) == pml[np.arange(B), winner]).all()  # the same doubles
    assert (np.asarray(st.crc_pass).astype(bool) == np.asarray(passed).astype(bool)).all()
