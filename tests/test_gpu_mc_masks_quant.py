"""The Monte-Carlo generator (csrc/qpd_mc.hip: mc_frames_kernel in its four modes, mc_count_kernel)
away from the one point every other test of it uses -- q = 16 on a uniform or MinDistortion
quantizer, a PW mask, K - A = 24, a seed below 2^32 -- on the case table of tests/mc_cases.py
(what the table covers is asserted on the CPU by tests/test_mc_cases.py):

(a) messages exactly, LLRs within the project's 2e-13 / sigma and, at sigma = 1e-3, the sign of
    every LLR against codes.polar_encode, on every mask and seed;
(b) the symbols of every quantizer = codes.quantize_channel of the device's own LLRs (exact: no
    allowance), in the symbol mode and as rec[symbol];
(c) quantizers whose edges ARE device LLRs: llr == edge on hundreds of positions;
(d) qpd_mc_decode = qpd_mc_frames + decode = the CPU oracle, for other alphabets, q < v, decoders
    without the root pre-pass and CRC tails shorter than the register;
(e) the device counters against a host count, added to a non-zero start, on every branch of
    mc_count_kernel;
and the alignment contract of d_msg (include/qpd.h)."""
import ctypes

import numpy as np
import pytest

import code_masks as M
import mc_cases as T
import mc_ref
from test_float_oracle import CRC24

pytestmark = pytest.mark.gpu

FAST, GENERIC = 2, 1  # qpd_info.engine
ENV = ("QPD_NO_PFX", "QPD_NO_PRE", "QPD_NO_BFUSE", "QPD_LDS_BUDGET", "QPD_SETS", "QPD_PFX1B", "QPD_PRE_CHUNK")
MASKS = T.masks()


@pytest.fixture(scope="module")
def env(native_lib, oracle_mod):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import quantized_decoder_polar_codes_amd as Q
    from quantized_decoder_polar_codes_amd import _lib
    from quantized_decoder_polar_codes_amd import codes as C
    from quantized_decoder_polar_codes_amd import lut as LU
    from quantized_decoder_polar_codes_amd import lutgen as LG
    from quantized_decoder_polar_codes_amd import montecarlo as MC
    from quantized_decoder_polar_codes_amd.decoders import from_quant

    class Env:
        pass

    e = Env()
    e.torch, e.lib, e.L, e.C, e.LU, e.LG, e.MC, e.Q, e.from_quant = torch, native_lib, _lib, C, LU, LG, MC, Q, from_quant
    e.oracle = oracle_mod
    e.quantizers = T.quantizers(LG)
    return e


def _set_env(monkeypatch, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _code_of(env, fm):
    """A float SC decoder on the mask: the generator reads the code (N, mask) of any decoder kind."""
    fm = np.asarray(fm)
    K = int((fm == 0).sum())
    return env.from_quant("SC", fm.size, K, fm), np.flatnonzero(fm == 0), K


def _pw(env, N, K):
    _, mb, fm, _ = env.C.construct_pw(N, K)
    return np.asarray(fm, dtype=np.int64)


def _bits_equal(a, b):
    """Doubles bit for bit (-0.0 is not 0.0)."""
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


# ---------------------------------------------------------------------------------------------------------
# (a) messages and code words on every mask and seed
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family,name,fm", MASKS, ids=T.mask_ids())
def test_messages_llrs_and_code_words(env, family, name, fm):
    dec, mb, K = _code_of(env, fm)
    N = fm.size
    B = 8 if family == "big" else 96
    sigma = env.MC.sigma_for(2.0, K / N)
    e16, l16 = env.MC.uniform_channel_quantizer(16, 0.5)
    for i, seed in enumerate(T.SEEDS):
        f0 = (0, 5, (1 << 33) + 17)[i]
        msg, llr = env.MC.GpuLlrFrames(dec, sigma, seed)(f0, B)
        msg_s, sym = env.MC.GpuFrames(dec, e16, l16, 16, sigma, seed)(f0, B)
        msg_q, quiet = env.MC.GpuLlrFrames(dec, 1e-3, seed)(f0, B)
        env.torch.cuda.synchronize()
        rmsg, _, rllr = mc_ref.frames(N, K, mb, seed, f0, B, sigma, e16, l16, 16)
        msg = msg.cpu().numpy()
        assert msg.shape == (B, K)
        assert np.array_equal(msg, rmsg), (name, hex(seed))
        assert np.array_equal(msg_s.cpu().numpy(), rmsg) and np.array_equal(msg_q.cpu().numpy(), rmsg)
        llr = llr.cpu().numpy()
        err = float(np.abs(llr - rllr).max())
        print(f"{name} seed {seed:#x}: max |llr - restatement| = {err:.3e} (bound {2e-13 / sigma:.3e})")
        assert err <= 2e-13 / sigma
        assert np.array_equal(sym.cpu().numpy(), env.C.quantize_channel(llr, e16, l16, 16))
        # no tolerance: at sigma = 1e-3 the noise cannot turn a sign
        x = env.C.polar_encode(rmsg, mb, N)
        assert np.array_equal(quiet.cpu().numpy() > 0, x == 0), (name, hex(seed))
    # the seed's high word counts
    m_lo, _ = env.MC.GpuLlrFrames(dec, sigma, T.SEEDS[1] & 0xFFFFFFFF)(0, B)
    m_hi, _ = env.MC.GpuLlrFrames(dec, sigma, T.SEEDS[1])(0, B)
    if B * K >= 64:
        assert not env.torch.equal(m_lo, m_hi)


# ---------------------------------------------------------------------------------------------------------
# (b) symbols on every quantizer
# ---------------------------------------------------------------------------------------------------------

QN, QK, QB, QF0 = 256, 128, 96, 1000
QSEED = T.SEEDS[1]
SIGMAS = (0.8, 0.25)  # LLRs of about +-3 +- 2.5 and of +-32 +- 8: both ends of the narrow and of the +-50 quantizers


def _rec_for(q, seed=9):
    rec = np.random.default_rng(seed).normal(0, 5, size=q)
    assert np.unique(rec).size == q
    return rec


def _check_quantizer(env, dec, edges, lut, q, sigma, with_rec=True, seed=QSEED, f0=QF0, B=QB):
    """Symbol mode and rec mode against quantize_channel of the device's own LLRs; returns (llr, symbols)."""
    msg_l, llr = env.MC.GpuLlrFrames(dec, sigma, seed)(f0, B)
    msg_s, sym = env.MC.GpuFrames(dec, edges, lut, q, sigma, seed)(f0, B)
    env.torch.cuda.synchronize()
    llr, sym = llr.cpu().numpy(), sym.cpu().numpy()
    assert env.torch.equal(msg_l, msg_s)
    want = env.C.quantize_channel(llr, edges, lut, q)
    bad = np.argwhere(sym != want)
    assert bad.size == 0, (len(bad), [(llr[i, j].hex(), int(sym[i, j]), int(want[i, j])) for i, j in bad[:5]])
    if with_rec:
        rec = _rec_for(q)
        msg_r, rl = env.MC.GpuLlrFrames(dec, sigma, seed, edges, lut, q, rec=rec)(f0, B)
        env.torch.cuda.synchronize()
        assert env.torch.equal(msg_l, msg_r)
        assert _bits_equal(rl.cpu().numpy(), rec[want])
    return llr, sym


@pytest.mark.parametrize("name", sorted(T.quantizers()) + ["mindistortion"])
def test_symbols_on_every_quantizer(env, name):
    edges, lut, q = env.quantizers[name]
    dec, _, _ = _code_of(env, _pw(env, QN, QK))
    seen = set()
    for sigma in SIGMAS:
        llr, sym = _check_quantizer(env, dec, edges, lut, q, sigma, with_rec=name not in T.SYMBOL_MODE_ONLY)
        seen |= set(np.unique(sym).tolist())
        if (llr <= edges[0]).any():
            seen.add("low")
        if (llr >= edges[-1]).any():
            seen.add("high")
    if max(abs(edges[0]), abs(edges[-1])) <= 50:  # every quantizer but `wide` and `overflow`
        assert {"low", "high", 0, q - 1} <= seen, name
    else:
        assert "low" not in seen and "high" not in seen
    if edges[0] < edges[-1]:  # `allequal` has no inner LLR
        inner = set(np.asarray(lut).tolist())
        assert len(seen & inner) >= min(len(inner), 2)


def test_q300_is_refused_with_rec(env):
    edges, lut, q = env.quantizers["q300"]
    dec, _, _ = _code_of(env, _pw(env, QN, QK))
    src = env.MC.GpuLlrFrames(dec, 0.8, QSEED, edges, lut, q, rec=np.linspace(-1, 1, q))
    with pytest.raises(ValueError, match="256"):
        src(0, 8)
    assert dec.info()["last_engine"] == env.L.QPD_RAN_NONE


# ---------------------------------------------------------------------------------------------------------
# (c) LLRs exactly on edges
# ---------------------------------------------------------------------------------------------------------

def test_llrs_exactly_on_edges(env):
    """Edges taken from the LLRs the generator will produce (same seed, same range): llr == edge on every
    inner edge of a 256-bin table, on both outer edges, next to an edge on either side, and on a tripled edge."""
    sigma = 0.8
    dec, _, _ = _code_of(env, _pw(env, QN, QK))
    _, dl = env.MC.GpuLlrFrames(dec, sigma, QSEED)(QF0, QB)
    env.torch.cuda.synchronize()
    dl = dl.cpu().numpy()
    vals = np.unique(dl)
    assert vals.size >= 20000
    rng = np.random.default_rng(77)
    # 257 distinct sample values across the sorted sample, the smallest and the largest included
    e1 = vals[np.round(np.linspace(0, vals.size - 1, 257)).astype(np.int64)]
    assert np.unique(e1).size == 257 and e1[0] == dl.min() and e1[-1] == dl.max()
    l1 = T.scrambled_lut(256, 16, rng)
    x = vals[vals.size // 2 + 3]  # a chosen value: an LLR near the median
    e2 = np.array([vals[0], np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf), vals[-1]])
    e3 = np.array([vals[0], x, x, x, vals[-1]])
    for edges, lut, q in ((e1, l1, 16), (e2, np.array([2, 0, 3, 1], dtype=np.int32), 4),
                          (e3, np.array([1, 3, 0, 2], dtype=np.int32), 4)):
        llr, sym = _check_quantizer(env, dec, edges, lut, q, sigma)
        assert _bits_equal(llr, dl)  # the same doubles as the edges were taken from
        assert (llr == edges[0]).sum() >= 1 and (sym[llr == edges[0]] == 0).all()
        assert (llr == edges[-1]).sum() >= 1 and (sym[llr == edges[-1]] == q - 1).all()
    # coverage of the 256-bin table, counted on the device's LLRs
    inner = e1[1:-1]
    differ = l1[:-1] != l1[1:]  # the bins on either side of inner edge i map to different symbols
    on_edge = np.isin(dl, inner[differ])
    assert int(on_edge.sum()) >= 200
    # llr == inner edge i belongs to the bin below it (bisect_left): lut[i]
    idx = np.searchsorted(e1, dl[on_edge])
    want = l1[idx - 1]
    got = env.MC.GpuFrames(dec, e1, l1, 16, sigma, QSEED)(QF0, QB)[1].cpu().numpy()[on_edge]
    assert np.array_equal(got, want)
    assert (dl == x).sum() >= 1


# ---------------------------------------------------------------------------------------------------------
# (d) fused = unfused = oracle
# ---------------------------------------------------------------------------------------------------------

def _quantizer_for(env, q):
    if q in (2, 3, 8, 15, 16):
        return T.uniform_q(q)
    e, _ = env.MC.uniform_channel_quantizer(q, 8.0 / q)
    return e, T.scrambled_lut(q, q, np.random.default_rng(q)), q


def _three_way(env, kind, fm, v, q, engine="auto", ran=FAST, fused=None, chunks=1, A=None, B=96, f0=40, seed=T.SEEDS[2],
               tseed=0):
    """decode_frames = decode_batch(symbols of __call__) = the oracle on those symbols; the engine, and the
    generator's launches (one per chunk).  fused: which branch of mc_decode must have run, told by the root
    pre-pass launches (decode_batch makes one per chunk on a pre-mode decoder, the fused call none: the generator
    writes the pre-pass rows itself); "auto": fused if the decoder is in pre-mode.  Returns (decoder, messages,
    whether the fused branch ran)."""
    fm = np.asarray(fm)
    N, K = fm.size, int((fm == 0).sum())
    nt = M.node_type_of(fm)
    L = 1 if kind == "SC-LUT" else 8
    p = env.LU.random_luts(N, v, seed=100 * N + v + tseed, distinct_mags=3)
    kw = {} if A is None else {"A": A}
    dec = env.Q.from_packed(kind, p, K, fm, L=L, node_type=nt, engine=engine, **kw)
    if ran is not None:
        assert dec.info()["engine"] == ran, (kind, N, dec.info()["engine"])
    edges, lut, _ = _quantizer_for(env, q)
    sigma = env.MC.sigma_for(2.0, K / N)
    src = env.MC.GpuFrames(dec, edges, lut, q, sigma, seed)
    dec.profile(True)
    dec.kernel_times()
    msg_a, sym = src(f0, B)
    env.torch.cuda.synchronize()
    assert dec.kernel_times()["mc"][1] == 1
    bits_u = dec.decode_batch(sym)
    env.torch.cuda.synchronize()
    pre_unfused = dec.kernel_times()["pre"][1]
    msg_b, bits_f = src.decode_frames(f0, B)
    env.torch.cuda.synchronize()
    kt = dec.kernel_times()
    assert kt["mc"][1] == chunks, kt
    pre_mode = pre_unfused >= 1
    if fused is True:
        assert pre_mode, "not a pre-mode decoder"
    if fused is False:
        assert kt["pre"][1] == pre_unfused, (kt, pre_unfused)
    elif pre_mode and dec.info()["engine"] == FAST:
        assert kt["pre"][1] == 0, kt
    assert dec.info()["last_engine"] == env.L.QPD_RAN_GPU
    sym_h = sym.cpu().numpy()
    assert sym_h.min() >= 0 and sym_h.max() < q
    if A is None:
        want = env.oracle.decode_lut(kind, p, K, L, fm, sym_h, node_type=nt)
    else:
        want = env.oracle.decode_lut_ca(kind, p, K, A, L, fm, sym_h, node_type=nt)
    assert env.torch.equal(msg_a, msg_b)
    label = f"{kind}-N{N}-v{v}-q{q}-{engine}"
    assert np.array_equal(bits_u.cpu().numpy(), want), label + " unfused"
    assert np.array_equal(bits_f.cpu().numpy(), want), label + " fused"
    return dec, msg_a.cpu().numpy(), pre_mode and fused is not False


VQ = [(2, 2), (3, 3), (8, 8), (15, 15), (16, 16), (16, 8), (3, 2)]
FUSED_KINDS = ["SC-LUT", "SCL-LUT", "FastSCL-LUT", "CA-SCL-LUT"]


def _fused_codes(env):
    out = [_pw(env, 64, 32), M.block_mask(64, M.BLOCK_SEEDS[64][0]), _pw(env, 256, 128),
           M.block_mask(256, M.BLOCK_SEEDS[256][0])]
    return out


@pytest.mark.parametrize("v,q", VQ)
@pytest.mark.parametrize("kind", FUSED_KINDS)
def test_fused_equals_unfused_equals_oracle(env, monkeypatch, kind, v, q):
    """q <= v on a fast-engine decoder in pre-mode: the generator writes the root pre-pass rows."""
    _set_env(monkeypatch, {})
    ran_fused = []
    for fm in _fused_codes(env):
        assert not M.special_root(fm, kind)
        K = int((fm == 0).sum())
        ran_fused.append(_three_way(env, kind, fm, v, q, fused="auto", A=K - 24 if kind.startswith("CA-") else None)[2])
    assert ran_fused[0] and ran_fused[2], ran_fused  # the PW codes are pre-mode decoders


def test_fused_chunks_launch_the_generator_once_each(env, monkeypatch):
    _set_env(monkeypatch, {"QPD_PRE_CHUNK": "40"})
    _three_way(env, "SCL-LUT", _pw(env, 256, 128), 8, 8, fused=True, chunks=3)  # 96 frames: 40 + 40 + 16


def test_q_above_v_takes_the_unfused_branch_and_is_flagged(env, monkeypatch):
    """q = 16 on v = 8: the symbols go through a buffer and the decode's own range check, which reports them."""
    _set_env(monkeypatch, {})
    N, K, v, q = 256, 128, 8, 16
    fm = _pw(env, N, K)
    p = env.LU.random_luts(N, v, seed=3, distinct_mags=3)
    dec = env.Q.from_packed("SCL-LUT", p, K, fm, L=8, node_type=M.node_type_of(fm))
    assert dec.info()["engine"] == FAST
    edges, lut, _ = T.uniform_q(q)
    src = env.MC.GpuFrames(dec, edges, lut, q, env.MC.sigma_for(2.0, K / N), T.SEEDS[0])
    _, sym = src(0, 96)
    assert int(sym.max()) >= v
    dec.profile(True)
    dec.kernel_times()
    src.decode_frames(0, 96)
    with pytest.raises(ValueError, match="outside"):
        env.L.check(env.lib.qpd_check_input_error(dec._h))
    kt = dec.kernel_times()
    assert kt["mc"][1] == 1 and kt["pre"][1] == 1, kt  # the decode ran its own root pre-pass


UNFUSED = [
    # kind, (N, mask or K), v, q, engine, switches, engine that runs
    ("SCL-LUT", (8, 4), 16, 16, "auto", {}, None),                      # N < 16: no root pre-pass
    ("SC-LUT", (8, 4), 8, 8, "auto", {}, None),
    ("FastSCL-LUT", (64, "antipolar"), 16, 16, "auto", {}, None),       # the root's left child is an R1 node
    ("SCL-LUT", (256, 128), 16, 16, "auto", {"QPD_NO_PRE": "1"}, FAST),
    ("FastSCL-LUT", (256, 128), 8, 8, "auto", {"QPD_NO_PRE": "1"}, FAST),
    ("SCL-LUT", (256, 128), 16, 16, "generic", {}, GENERIC),
    ("CA-SCL-LUT", (256, 128), 8, 8, "generic", {}, GENERIC),
    ("SCL-LUT", (64, 32), 32, 32, "auto", {}, GENERIC),                 # v > 16: the generic engine
    ("SC-LUT", (64, 32), 32, 32, "auto", {}, GENERIC),
]


@pytest.mark.parametrize("kind,code,v,q,engine,switches,ran", UNFUSED,
                         ids=[f"{c[0]}-{c[1][0]}-{c[1][1]}-v{c[2]}-{c[4]}{'-'.join(c[5])}" for c in UNFUSED])
def test_unfused_branch_of_mc_decode(env, monkeypatch, kind, code, v, q, engine, switches, ran):
    """Decoders without the root pre-pass: qpd_mc_decode generates symbols into its own buffer."""
    _set_env(monkeypatch, switches)
    N, second = code
    fm = M.named_mask(N, second) if isinstance(second, str) else _pw(env, N, second)
    assert not M.special_root(fm, kind)
    K = int((fm == 0).sum())
    _three_way(env, kind, fm, v, q, engine=engine, ran=ran, fused=False, A=K - 24 if kind.startswith("CA-") else None)


@pytest.mark.parametrize("K,A", T.CRC_CASES)
def test_crc_tails(env, monkeypatch, K, A):
    """K - A < crc_n: the message is followed by the first K - A bits of its CRC (the top of the register).
    Messages exactly; the code word -- CRC bits included -- through the LLRs' bound and signs; three ways."""
    _set_env(monkeypatch, {})
    N = 128
    fm = _pw(env, N, K)
    mb = np.flatnonzero(fm == 0)
    dec, msg, _ = _three_way(env, "CA-SCL-LUT", fm, 16, 16, fused="auto", A=A, seed=T.SEEDS[1])
    assert dec.info()["out_bits"] == A
    crc = (T.CRC_N, CRC24)
    sigma = 0.7
    e16, l16 = env.MC.uniform_channel_quantizer(16, 0.5)
    rmsg, _, rllr = mc_ref.frames(N, K, mb, T.SEEDS[1], 40, 96, sigma, e16, l16, 16, A=A, crc=crc)
    assert np.array_equal(msg, rmsg)
    m2, llr = env.MC.GpuLlrFrames(dec, sigma, T.SEEDS[1])(40, 96)
    m3, quiet = env.MC.GpuLlrFrames(dec, 1e-3, T.SEEDS[1])(40, 96)
    env.torch.cuda.synchronize()
    assert np.array_equal(m2.cpu().numpy(), rmsg) and np.array_equal(m3.cpu().numpy(), rmsg)
    assert float(np.abs(llr.cpu().numpy() - rllr).max()) <= 2e-13 / sigma
    u = np.concatenate([rmsg, env.oracle.crc_encode(rmsg, T.CRC_N, CRC24)[:, : K - A]], axis=1)
    assert u[:, A:].any() and not u[:, A:].all()
    assert np.array_equal(quiet.cpu().numpy() > 0, env.C.polar_encode(u, mb, N) == 0)


# ---------------------------------------------------------------------------------------------------------
# (e) counters, and the alignment of d_msg
# ---------------------------------------------------------------------------------------------------------

def _channel(env, edges, lut, q, sigma):
    ch = env.L.QpdMcChannel()
    ch.sigma, ch.q, ch.n_edges, ch.edges, ch.lut = sigma, q, len(edges), edges.ctypes.data, lut.ctypes.data
    return ch


def _mc_decode(env, dec, ch, seed, f0, B, msg_ptr, out_ptr, counts):
    P = ctypes.c_void_p
    rc = env.lib.qpd_mc_decode(dec._h, ctypes.byref(ch), ctypes.c_uint64(seed), f0, B, P(msg_ptr), P(out_ptr),
                               None if counts is None else P(counts.data_ptr()), None)
    env.torch.cuda.synchronize()
    return rc, env.lib.qpd_last_error().decode()


def _count_decoder(env, out_bits):
    if out_bits >= 1000:
        N = 2048
        fm = T.pw_big(N, out_bits)
    elif out_bits >= 512:
        N, fm = 1024, _pw(env, 1024, out_bits)
    elif out_bits == 1:
        N, fm = 16, M.named_mask(16, "K1_mid")
    else:
        N, fm = 32, _pw(env, 32, out_bits)
    return env.Q.from_packed("SC-LUT", env.LU.minsum_uniform_luts(N), out_bits, fm), N


# out_bits: 1000 the 8-byte branch beyond one step per lane (K > 512), 1001 the byte branch there, 512 the
# one-step branch at its limit, 520 just past it, 8 one active lane, 1 the byte branch with one byte
@pytest.mark.parametrize("out_bits", [1000, 1001, 512, 520, 8, 1])
def test_counters_are_added_to(env, monkeypatch, out_bits):
    _set_env(monkeypatch, {})
    torch = env.torch
    dec, N = _count_decoder(env, out_bits)
    assert dec.out_bits == out_bits
    B = 64 if N == 2048 else 96
    e16, l16 = env.MC.uniform_channel_quantizer(16, 0.5)
    sigma = env.MC.sigma_for(1.0 if out_bits > 8 else -2.0, out_bits / N)
    counts = torch.tensor([7, 3], dtype=torch.int64, device="cuda")
    src = env.MC.GpuFrames(dec, e16, l16, 16, sigma, T.SEEDS[1])
    msg, bits = src.decode_frames(11, B, counts=counts)
    torch.cuda.synchronize()
    diff = (bits != msg).cpu().numpy()
    be, fe = int(diff.sum()), int(diff.any(1).sum())
    assert fe > 0 and be >= fe
    assert counts.tolist() == [7 + be, 3 + fe]
    msg2, bits2 = src.decode_frames(11, B, counts=counts)  # and once more on top
    torch.cuda.synchronize()
    assert torch.equal(bits, bits2) and counts.tolist() == [7 + 2 * be, 3 + 2 * fe]
    quiet = env.MC.GpuFrames(dec, e16, l16, 16, 1e-3, T.SEEDS[1])
    msg3, bits3 = quiet.decode_frames(11, B, counts=counts)
    torch.cuda.synchronize()
    assert torch.equal(msg3, bits3) and counts.tolist() == [7 + 2 * be, 3 + 2 * fe]


def test_counters_with_d_out_one_byte_off(env, monkeypatch):
    """out_bits = 512 and d_out one byte past an aligned base: mc_count_kernel's byte branch, the same counts
    (d_msg must be aligned -- below -- so d_out is the only way into that branch at a multiple of 8)."""
    _set_env(monkeypatch, {})
    torch = env.torch
    dec, N = _count_decoder(env, 512)
    B, f0, seed = 96, 11, T.SEEDS[1]
    e16, l16 = env.MC.uniform_channel_quantizer(16, 0.5)
    ch = _channel(env, e16, l16, 16, env.MC.sigma_for(1.0, 0.5))
    got = []
    for off in (0, 1):
        msg = torch.zeros((B, 512), dtype=torch.uint8, device="cuda")
        flat = torch.full((B * 512 + 16,), 9, dtype=torch.uint8, device="cuda")
        counts = torch.tensor([7, 3], dtype=torch.int64, device="cuda")
        assert msg.data_ptr() % 8 == 0 and flat.data_ptr() % 8 == 0
        rc, why = _mc_decode(env, dec, ch, seed, f0, B, msg.data_ptr(), flat.data_ptr() + off, counts)
        assert rc == env.L.QPD_OK, why
        out = flat[off: off + B * 512].view(B, 512)
        assert bool((flat[:off] == 9).all()) and bool((flat[off + B * 512:] == 9).all())
        diff = (out != msg).cpu().numpy()
        assert counts.tolist() == [7 + int(diff.sum()), 3 + int(diff.any(1).sum())] and diff.any()
        got.append((out.clone(), counts.tolist()))
    assert torch.equal(got[0][0], got[1][0]) and got[0][1] == got[1][1]


def test_misaligned_d_msg_is_refused(env, monkeypatch):
    """include/qpd.h: rows of a multiple of 8 message bits need an 8-byte aligned d_msg (the generator stores
    them 8 bytes at a time) -- QPD_E_INVALID from all four entry points before anything is launched; any base
    serves other row lengths."""
    _set_env(monkeypatch, {})
    torch, L = env.torch, env.L
    P = ctypes.c_void_p
    N, K, B = 128, 64, 8
    fm = _pw(env, N, K)
    e16, l16 = env.MC.uniform_channel_quantizer(16, 0.5)
    ch = _channel(env, e16, l16, 16, 0.8)
    lut_dec = env.Q.from_packed("SC-LUT", env.LU.minsum_uniform_luts(N), K, fm)
    flt_dec = env.from_quant("SC", N, K, fm)
    flat = torch.full((B * K + 8,), 9, dtype=torch.uint8, device="cuda")
    out = torch.full((B * K,), 9, dtype=torch.uint8, device="cuda")
    sym = torch.full((B * N,), -7, dtype=torch.int32, device="cuda")
    llr = torch.full((B * N,), -1.5, dtype=torch.float64, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    seed = ctypes.c_uint64(5)
    for off in (1, 4, 7):
        bad = P(flat.data_ptr() + off)
        calls = [
            (lut_dec, lambda: env.lib.qpd_mc_frames(lut_dec._h, ctypes.byref(ch), seed, 0, B, bad, P(sym.data_ptr()), None)),
            (lut_dec, lambda: env.lib.qpd_mc_decode(lut_dec._h, ctypes.byref(ch), seed, 0, B, bad, P(out.data_ptr()),
                                                    P(counts.data_ptr()), None)),
            (flt_dec, lambda: env.lib.qpd_mc_llr(flt_dec._h, ctypes.byref(ch), None, seed, 0, B, bad, P(llr.data_ptr()), None)),
            (flt_dec, lambda: env.lib.qpd_mc_decode_f64(flt_dec._h, ctypes.byref(ch), None, seed, 0, B, bad,
                                                        P(out.data_ptr()), P(counts.data_ptr()), None)),
        ]
        for dec, call in calls:
            assert call() == L.QPD_E_INVALID
            assert "alignment" in env.lib.qpd_last_error().decode()
            assert dec.info()["last_engine"] == L.QPD_RAN_NONE
    torch.cuda.synchronize()
    assert bool((flat == 9).all()) and bool((out == 9).all()) and bool((sym == -7).all()) and bool((llr == -1.5).all())
    assert counts.tolist() == [0, 0]
    # a row length off the 8-byte grid takes any base, and gives the aligned call's bits
    K2 = 61
    fm2 = _pw(env, N, K2)
    dec2 = env.from_quant("SC", N, K2, fm2)
    want, _ = env.MC.GpuLlrFrames(dec2, 0.8, 5)(0, B)
    for off in (1, 3):
        flat2 = torch.full((B * K2 + 8,), 9, dtype=torch.uint8, device="cuda")
        rc = env.lib.qpd_mc_llr(dec2._h, ctypes.byref(ch), None, seed, 0, B, P(flat2.data_ptr() + off), P(llr.data_ptr()), None)
        torch.cuda.synchronize()
        assert rc == L.QPD_OK
        assert torch.equal(flat2[off: off + B * K2].view(B, K2), want)
        assert bool((flat2[:off] == 9).all()) and bool((flat2[off + B * K2:] == 9).all())
