"""Rows in lookup order (QPD_ROW_BYTEIDX, csrc/qpd_fast_switches.hpp): the plain kinds keep every S row of
M >= 8 symbols with element k in the high nibble of byte k mod 4 of word k / 4 and element k + M/2 in the low
one, so an f / g op reads its table indices as they lie.  Every producer and consumer of such a row must agree
on the order -- the pre-pass (int32, uint8, LLR input, the Monte-Carlo generator), gsel_op, fg_op, ff_op, the
folded and unfolded BOT3, the prefix stages' exports and imports -- and the bits must stay the oracle's.

The shapes are the smallest at which each path first appears: N = 16 (one op of M = 16 above BOT3, or the fold
alone), N = 32 / 64 (multi-word rows, folded descents), N = 1024 (slab rows, both prefix stages, MF_GSEL);
with one frame set and without the prefix stages / the pre-pass; SC-LUT, CA-SCL-LUT, W16; the other inputs;
FastSCL-LUT, whose rows keep the element order.  Alphabets of 16 and 8 symbols, a frozen mask that is no
reliability order's, and random tables, which are asymmetric: a case counts only if the oracle itself decodes
other bits from the tables with a and b swapped (f(b, a), g(b, a, u)), so a swapped nibble pair cannot pass.
"""
import numpy as np
import pytest

import code_masks as M
import mc_cases as T
from conftest import assert_frames_equal

pytestmark = pytest.mark.gpu

ENV = ("QPD_SETS", "QPD_NO_PFX", "QPD_NO_PRE")


@pytest.fixture(scope="module")
def env(native_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import quantized_decoder_polar_codes_amd as Q
    from quantized_decoder_polar_codes_amd import codes as C
    from quantized_decoder_polar_codes_amd import lut as LU
    from quantized_decoder_polar_codes_amd import montecarlo as MC

    class Env:
        pass

    e = Env()
    e.torch, e.Q, e.C, e.LU, e.MC = torch, Q, C, LU, MC
    return e


def _mask(env, N, K, mask):
    if mask == "pw":
        _, _, fm, _ = env.C.construct_pw(N, K)
    else:  # K information positions drawn uniformly: nested in no reliability order
        fm = M.random_mask(N, K, 17 * N + K)
    return np.asarray(fm)


def _swapped(LU, p):
    """p with a and b exchanged in every f and g table."""
    return LU.PackedLUT(N=p.N, v=p.v, lut_f=np.ascontiguousarray(p.lut_f.swapaxes(-1, -2)), f_base=p.f_base,
                        f_step=p.f_step, lut_g=np.ascontiguousarray(p.lut_g.swapaxes(-1, -2)), g_base=p.g_base,
                        g_step=p.g_step, vcl=p.vcl)


def _case(env, oracle_mod, kind, N, K, L, v, mask, B, A=None):
    """(tables, frozen mask, node types, symbols, the oracle's bits) of a case whose tables tell a from b."""
    fm = _mask(env, N, K, mask)
    nt = M.node_type_of(fm)
    base = kind[3:] if kind.startswith("CA-") else kind

    def want_of(p, sym):
        if A is not None:
            return oracle_mod.decode_lut_ca(kind, p, K, A, L, fm, sym, node_type=nt)
        return oracle_mod.decode_lut(base, p, K, L, fm, sym, node_type=nt)

    for seed in range(8):  # (other seeds if a table set happens not to tell)
        p = env.LU.random_luts(N, v, seed=1000 * N + 10 * v + seed, distinct_mags=3)
        sym = np.random.default_rng(N + K + seed).integers(0, v, size=(B, N), dtype=np.int32)
        want = want_of(p, sym)
        if (want_of(_swapped(env.LU, p), sym) != want).any():
            return p, fm, nt, sym, want
    raise AssertionError(f"{kind} N={N}: no table seed tells f(a, b) from f(b, a)")


def _set_env(monkeypatch, mode):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, val in {"default": {}, "sets1": {"QPD_SETS": "1"}, "nopfx": {"QPD_NO_PFX": "1"}, "nopre": {"QPD_NO_PRE": "1"}}[mode].items():
        monkeypatch.setenv(k, val)


def _decode_and_check(env, oracle_mod, monkeypatch, kind, N, K, L, v, mask, B, mode, A=None, label=""):
    p, fm, nt, sym, want = _case(env, oracle_mod, kind, N, K, L, v, mask, B, A=A)
    _set_env(monkeypatch, mode)
    kw = {} if A is None else {"A": A}
    dec = env.Q.from_packed(kind, p, K, fm, L=L, node_type=nt, engine="fast", **kw)
    got = dec.decode_batch(env.torch.from_numpy(sym).cuda()).cpu().numpy()
    assert_frames_equal(got, want, dec, f"row-order-{label or kind}-N{N}-v{v}-{mask}-{mode}")
    return dec, p, fm, nt, sym, want


# N = 16: one op of M = 16 above BOT3, or the fold alone; N = 32: the first multi-word rows and folded descents
@pytest.mark.parametrize("N,K,v,mask", [(16, 8, 16, "pw"), (16, 9, 8, "random"), (32, 16, 16, "pw"), (32, 13, 8, "random")])
def test_scl_small_codes(N, K, v, mask, env, oracle_mod, monkeypatch):
    _decode_and_check(env, oracle_mod, monkeypatch, "SCL-LUT", N, K, 8, v, mask, 96, "default")


@pytest.mark.parametrize("mode", ["default", "sets1", "nopfx", "nopre"])
@pytest.mark.parametrize("K,v,mask", [(32, 16, "pw"), (29, 8, "random")])
def test_scl_n64(K, v, mask, mode, env, oracle_mod, monkeypatch):
    _decode_and_check(env, oracle_mod, monkeypatch, "SCL-LUT", 64, K, 8, v, mask, 96, mode)


@pytest.mark.parametrize("mode", ["default", "sets1", "nopfx", "nopre"])
@pytest.mark.parametrize("v,mask", [(16, "pw"), (8, "random")])
def test_scl_bench_code(v, mask, mode, env, oracle_mod, monkeypatch):
    """N = 1024, K = 512, 256 frames: slab rows, both prefix stages, MF_GSEL."""
    dec, *_ = _decode_and_check(env, oracle_mod, monkeypatch, "SCL-LUT", 1024, 512, 8, v, mask, 256, mode)
    if mode == "default" and mask == "pw":
        assert dec.info()["prefix_ops"] > 0


@pytest.mark.parametrize("v,mask", [(16, "pw"), (8, "random")])
def test_sc_lut(v, mask, env, oracle_mod, monkeypatch):
    _decode_and_check(env, oracle_mod, monkeypatch, "SC-LUT", 128, 32, 1, v, mask, 192, "default")


def test_ca_scl_lut(env, oracle_mod, monkeypatch):
    _decode_and_check(env, oracle_mod, monkeypatch, "CA-SCL-LUT", 64, 40, 8, 16, "pw", 96, "default", A=29)


@pytest.mark.parametrize("v,mask", [(16, "pw"), (8, "random")])
def test_scl_w16(v, mask, env, oracle_mod, monkeypatch):
    _decode_and_check(env, oracle_mod, monkeypatch, "SCL-LUT", 64, 32, 16, v, mask, 96, "default", label="W16")


def test_fastscl_keeps_element_order(env, oracle_mod, monkeypatch):
    _decode_and_check(env, oracle_mod, monkeypatch, "FastSCL-LUT", 64, 32, 8, 16, "pw", 96, "default")


def test_uint8_input(env, oracle_mod, monkeypatch):
    dec, p, fm, nt, sym, want = _decode_and_check(env, oracle_mod, monkeypatch, "SCL-LUT", 64, 32, 8, 16, "pw", 100, "default")
    got = dec.decode_batch(env.torch.from_numpy(sym.astype(np.uint8)).cuda()).cpu().numpy()
    assert_frames_equal(got, want, dec, "row-order-u8")
    assert dec.info()["u8_staged"] == 0  # read as they are by the pre-pass


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_llr_input(dtype, env, oracle_mod, monkeypatch):
    """The LLR front kernel writes the pre-pass rows: LLRs at the centres of the uniform quantizer's cells."""
    dec, p, fm, nt, sym, want = _decode_and_check(env, oracle_mod, monkeypatch, "SCL-LUT", 64, 32, 8, 16, "pw", 100, "default")
    edges, lut, q = T.uniform_q(16)
    cq = env.Q.ChannelQuantizer(edges, lut, q)
    edges = np.asarray(edges, dtype=np.float64)
    centres = 0.5 * (edges[:-1] + edges[1:])
    cells = np.array([int(np.flatnonzero(np.asarray(lut) == s)[0]) for s in range(16)])
    llr = centres[cells][sym]
    t = env.torch.from_numpy(llr).cuda()
    if dtype == "f32":
        t = t.to(env.torch.float32)
    got = dec.decode_llr_batch(t, cq).cpu().numpy()
    assert_frames_equal(got, want, dec, f"row-order-llr-{dtype}")


def test_generator_pre_rows(env, oracle_mod, monkeypatch):
    """decode_frames: the generator writes the pre-pass rows itself (MC_PRE); the bits are the oracle's on the
    symbols the generator gives for the same frames."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    N, K, L, B = 64, 32, 8, 96
    p, fm, nt, _, _ = _case(env, oracle_mod, "SCL-LUT", N, K, L, 16, "pw", 8)
    dec = env.Q.from_packed("SCL-LUT", p, K, fm, L=L, node_type=nt, engine="fast")
    edges, lut, q = T.uniform_q(16)
    src = env.MC.GpuFrames(dec, edges, lut, q, env.MC.sigma_for(2.0, K / N), T.SEEDS[0])
    _, sym = src(40, B)
    dec.profile(True)
    dec.kernel_times()
    _, bits = src.decode_frames(40, B)
    env.torch.cuda.synchronize()
    assert dec.kernel_times()["pre"][1] == 0  # the fused branch: no pre-pass launch
    want = oracle_mod.decode_lut("SCL-LUT", p, K, L, fm, sym.cpu().numpy(), node_type=nt)
    assert_frames_equal(bits.cpu().numpy(), want, dec, "row-order-mc-pre")
