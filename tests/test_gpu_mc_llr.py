"""GPU-resident Monte-Carlo for the float64-LLR decoders: qpd_mc_llr (the
generator's LLR output modes) and qpd_mc_decode_f64 (generate, decode_f64,
count, chunk by chunk), through montecarlo.GpuLlrFrames and simulate().

* the LLRs against the numpy restatement (tests/mc_ref.py), within the bound the
  device log / sin / cos allow; the messages exactly;
* exact, GPU against GPU: the LLRs quantized on the host are qpd_mc_frames'
  symbols bit for bit, and with a reconstruction table the output is rec[symbol];
* layout: sub-ranges, an 8-byte-aligned base, nothing written past the last row;
* the fused call equals generate + decode_batch for every float family, across a
  chunk seam too, and its device counters are the host's;
* refusals; simulate() on a float decoder; float and LUT decoders of one code get
  the same messages.
"""
import ctypes

import numpy as np
import pytest

from mc_ref import frames as ref_frames
from test_float_oracle import CRC24, quant_for

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(native_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import quantized_decoder_polar_codes_amd as Q  # noqa: F401
    from quantized_decoder_polar_codes_amd import _lib
    from quantized_decoder_polar_codes_amd import codes as C
    from quantized_decoder_polar_codes_amd import lutgen as LG
    from quantized_decoder_polar_codes_amd import montecarlo as MC
    from quantized_decoder_polar_codes_amd.decoders import from_quant

    class Env:
        pass

    e = Env()
    e.torch, e.lib, e.L, e.C, e.LG, e.MC, e.from_quant = torch, native_lib, _lib, C, LG, MC, from_quant
    return e


def _code(C, N, K):
    _, mb, fm, mm = C.construct_pw(N, K)
    return mb, fm, C.identify_nodes(N, mb).astype(np.int32)


def _float_decoder(env, kind, N, K, L=1, **kw):
    mb, fm, nt = _code(env.C, N, K)
    return env.from_quant(kind, N, K, fm, L=L, node_type=nt, quant=quant_for(kind, N), **kw), mb


# (N, K, frame0, B): N = 2 .. 64 run a partial wave; B = 5000 is more frames than one
# resident round of workgroups (the grid-stride loop, the LDS state carried across frames)
LLR_CASES = [(N, K, f0, 96) for N, K in [(2, 1), (8, 4), (16, 8), (64, 32), (64, 40), (256, 128), (1024, 512)]
             for f0 in (0, 5)] + [(64, 32, (1 << 33) + 17, 96), (64, 40, (1 << 33) + 17, 96), (64, 32, 0, 5000)]


@pytest.mark.parametrize("N,K,frame0,B", LLR_CASES)
def test_llrs_match_restatement(env, N, K, frame0, B):
    """msg exactly; |llr - restatement| <= 2e-13 / sigma: the device log / sin / cos are
    < 1 ulp each and the Box-Muller radius is at most sqrt(2 * 52 * ln 2) ~ 8.5, so
    |d nz| <~ 2e-14 and |d llr| <= (2 / sigma) |d nz|; the bound is 5x that."""
    dec, mb = _float_decoder(env, "SC", N, K)
    sigma = env.MC.sigma_for(2.0, K / N)
    src = env.MC.GpuLlrFrames(dec, sigma, seed=424242)
    msg, llr = src(frame0, B)
    env.torch.cuda.synchronize()
    assert msg.shape == (B, K) and llr.shape == (B, N) and llr.dtype == env.torch.float64
    edges, lut = env.MC.uniform_channel_quantizer(16, 0.5)
    rmsg, _, rllr = ref_frames(N, K, mb, 424242, frame0, B, sigma, edges, lut, 16)
    assert (msg.cpu().numpy() == rmsg).all()
    err = float(np.abs(llr.cpu().numpy() - rllr).max())
    print(f"max |llr - restatement| = {err:.3e} (bound {2e-13 / sigma:.3e}) N={N} K={K} frame0={frame0} B={B}")
    assert err <= 2e-13 / sigma


@pytest.mark.parametrize("quantizer", ["uniform", "mindistortion"])
def test_llrs_quantize_to_the_symbol_modes_symbols(env, quantizer):
    """The LLR mode stores the doubles the int32 mode bisects: quantized on the host
    they are its symbols, and with rec the output is rec[symbol], bit for bit."""
    N, K, B, f0 = 256, 128, 300, 1000
    dec, _ = _float_decoder(env, "SC", N, K)
    sigma = env.MC.sigma_for(2.0, K / N)
    if quantizer == "uniform":
        edges, lut = env.MC.uniform_channel_quantizer(16, 0.5)
    else:
        _, _, edges, lut = env.LG.channel_quantizer(sigma, 128, 16)
    msg_s, sym = env.MC.GpuFrames(dec, edges, lut, 16, sigma, seed=99)(f0, B)
    msg_l, llr = env.MC.GpuLlrFrames(dec, sigma, seed=99)(f0, B)
    rec = np.linspace(-7.5, 7.5, 16)
    msg_r, rl = env.MC.GpuLlrFrames(dec, sigma, 99, edges, lut, 16, rec=rec)(f0, B)
    env.torch.cuda.synchronize()
    assert env.torch.equal(msg_s, msg_l) and env.torch.equal(msg_s, msg_r)
    sym = sym.cpu().numpy()
    assert np.array_equal(env.C.quantize_channel(llr.cpu().numpy(), edges, lut, 16), sym)
    assert np.array_equal(rl.cpu().numpy(), rec[sym])
    assert sym.min() == 0 and sym.max() == 15  # both saturations were exercised


def test_subrange_agrees_on_the_overlap(env):
    dec, _ = _float_decoder(env, "SC", 256, 128)
    src = env.MC.GpuLlrFrames(dec, 0.8, seed=99)
    msg, llr = src(1000, 300)
    msg2, llr2 = src(1100, 50)
    env.torch.cuda.synchronize()
    assert env.torch.equal(msg[100:150], msg2) and env.torch.equal(llr[100:150], llr2)


@pytest.mark.parametrize("N,K", [(2, 1), (256, 128)])
@pytest.mark.parametrize("with_rec", [False, True])
def test_alignment_and_no_write_past_the_last_row(env, N, K, with_rec):
    """A base that is 8-byte but not 16-byte aligned gives the same doubles as an
    aligned one; the elements before the first and after the last row keep a sentinel."""
    torch = env.torch
    B, sentinel = 97, -12345.678
    dec, _ = _float_decoder(env, "SC", N, K)
    edges, lut = env.MC.uniform_channel_quantizer(16, 0.5)
    args = (edges, lut, 16, np.linspace(-7.5, 7.5, 16)) if with_rec else ()
    src = env.MC.GpuLlrFrames(dec, 0.9, 7, *args)
    flat_a = torch.full((B * N + 2,), sentinel, dtype=torch.float64, device=src.device)
    flat_u = torch.full((B * N + 3,), sentinel, dtype=torch.float64, device=src.device)
    assert flat_a.data_ptr() % 16 == 0 and flat_u[1:].data_ptr() % 16 == 8
    _, a = src(3, B, out=flat_a[: B * N])
    _, u = src(3, B, out=flat_u[1: 1 + B * N])
    torch.cuda.synchronize()
    assert torch.equal(a, u) and bool((a != sentinel).all())
    assert flat_a[B * N:].tolist() == [sentinel] * 2
    assert flat_u[0].item() == sentinel and flat_u[1 + B * N:].tolist() == [sentinel] * 2


def _rec_channel(env, sigma):
    """The drivers' MinDistortion channel quantizer with its quanta as reconstruction values."""
    _, quanta, edges, lut = env.LG.channel_quantizer(sigma, 128, 16)
    return edges, lut, 16, np.ascontiguousarray(quanta, dtype=np.float64)


FUSED_CASES = [("SC", 128, 32, 1, False), ("FastSC", 256, 128, 1, False), ("SCL", 128, 64, 4, False),
               ("SC-Uniform", 128, 64, 1, False), ("SCL-Lloyd", 128, 64, 2, True), ("CA-SCL", 256, 124, 8, False)]


@pytest.mark.parametrize("kind,N,K,L,with_rec", FUSED_CASES, ids=[c[0] for c in FUSED_CASES])
def test_fused_generate_decode_equals_unfused(env, kind, N, K, L, with_rec):
    """qpd_mc_decode_f64 = qpd_mc_llr followed by decode_batch, bit for bit; its device
    counters are the host's count; run_point with it gives the unfused counters."""
    torch, MC = env.torch, env.MC
    kw = dict(A=K - 24, crc_n=24, crc_loc=CRC24) if kind == "CA-SCL" else {}
    dec, _ = _float_decoder(env, kind, N, K, L, **kw)
    sigma = MC.sigma_for(1.0, K / N)
    src = MC.GpuLlrFrames(dec, sigma, 4321, *(_rec_channel(env, sigma) if with_rec else ()))
    msg_a, llr = src(5000, 3001)
    bits_a = dec.decode_batch(llr)
    counts = torch.zeros(2, dtype=torch.int64, device=src.device)
    msg_b, bits_b = src.decode_frames(5000, 3001, counts=counts)
    torch.cuda.synchronize()
    assert dec.info()["last_engine"] == env.L.QPD_RAN_GPU
    assert msg_a.shape == (3001, dec.out_bits)
    assert torch.equal(msg_a, msg_b)
    assert torch.equal(bits_a, bits_b)
    diff = bits_b != msg_b
    assert counts.tolist() == [int(diff.sum()), int(diff.any(1).sum())]
    for stop in (None, 50):
        a = MC.run_point(src, dec.decode_batch, dec.K, 1.0, 1000, 7000, stop, A=dec.out_bits, count_device=src.device)
        b = MC.run_point(src, dec.decode_batch, dec.K, 1.0, 1000, 7000, stop, A=dec.out_bits, count_device=src.device,
                         gen_decode=src.decode_frames)
        assert (a.bit_errors, a.block_errors, a.blocks, a.stopped_early) == \
            (b.bit_errors, b.block_errors, b.blocks, b.stopped_early)


def test_chunk_seam(env):
    """One call over more frames than a chunk of the LLR buffer holds (the rule of
    include/qpd.h): the frames around the seam and the last ones equal the unfused
    decode of those frame ids, and the counters cover the whole range."""
    torch, MC = env.torch, env.MC
    N, K, f0 = 1024, 512, 77
    chunk = MC.llr_chunk_frames(N)
    assert chunk == 2 ** 28 // (8 * 1024)
    B = chunk + 37
    dec, _ = _float_decoder(env, "FastSC", N, K)
    src = MC.GpuLlrFrames(dec, MC.sigma_for(1.5, K / N), seed=31)
    counts = torch.zeros(2, dtype=torch.int64, device=src.device)
    msg, bits = src.decode_frames(f0, B, counts=counts)
    for lo in (chunk - 80, B - 100):  # 100 frames around the seam (20 of them after it), the last 100
        assert 0 <= lo < chunk < lo + 100 <= B
        m, llr = src(f0 + lo, 100)
        assert torch.equal(m, msg[lo: lo + 100])
        assert torch.equal(dec.decode_batch(llr), bits[lo: lo + 100])
    diff = bits != msg
    assert counts.tolist() == [int(diff.sum()), int(diff.any(1).sum())]
    assert counts[1].item() > 0  # a channel with errors: the comparison above is not of zeros


def _call(env, name, dec, ch, rec, B, msg, buf, counts=None):
    P = ctypes.c_void_p
    fn = getattr(env.lib, name)
    args = [dec._h, ctypes.byref(ch), None if rec is None else P(rec.ctypes.data), ctypes.c_uint64(5), 0, B,
            P(msg.data_ptr()), P(buf.data_ptr())]
    if name == "qpd_mc_decode_f64":
        args.append(None if counts is None else P(counts.data_ptr()))
    rc = fn(*args, None)
    return rc, env.lib.qpd_last_error().decode()


def test_refusals(env):
    import quantized_decoder_polar_codes_amd as Q
    from quantized_decoder_polar_codes_amd import lut as LU

    torch, L = env.torch, env.L
    N, K, B = 128, 64, 8
    mb, fm, nt = _code(env.C, N, K)
    edges, lut = env.MC.uniform_channel_quantizer(16, 0.5)
    ch = L.QpdMcChannel()
    ch.sigma, ch.q, ch.n_edges, ch.edges, ch.lut = 0.8, 16, len(edges), edges.ctypes.data, lut.ctypes.data
    msg = torch.full((B, 256), 7, dtype=torch.uint8, device="cuda")
    out = torch.full((B, 256), 7, dtype=torch.uint8, device="cuda")
    llr = torch.full((B, 256), -1.5, dtype=torch.float64, device="cuda")
    # a LUT decoder: generating LLRs is fine (the code is what counts), decoding them is not
    lut_dec = Q.from_packed("SC-LUT", LU.minsum_uniform_luts(N), K, fm)
    assert _call(env, "qpd_mc_llr", lut_dec, ch, None, B, msg, llr)[0] == L.QPD_OK
    rc, why = _call(env, "qpd_mc_decode_f64", lut_dec, ch, None, B, msg, out)
    assert rc == L.QPD_E_INVALID and why
    # a reconstruction table with a NaN; a channel without sigma
    dec, _ = _float_decoder(env, "SC", N, K)
    rec = np.linspace(-7.5, 7.5, 16)
    rec[3] = np.nan
    for name, buf in (("qpd_mc_llr", llr), ("qpd_mc_decode_f64", out)):
        rc, why = _call(env, name, dec, ch, rec, B, msg, buf)
        assert rc == L.QPD_E_INVALID and "rec" in why
    bad = L.QpdMcChannel()
    bad.sigma = 0.0
    assert _call(env, "qpd_mc_llr", dec, bad, None, B, msg, llr)[0] == L.QPD_E_INVALID
    # CA-SCL float compares exactly crc_n bits; the generator has K - A CRC bits to give
    ca = env.from_quant("CA-SCL", 256, 130, _code(env.C, 256, 130)[1], L=2, A=100, crc_n=24, crc_loc=CRC24)
    for name, buf in (("qpd_mc_llr", llr), ("qpd_mc_decode_f64", out)):
        rc, why = _call(env, name, ca, ch, None, B, msg, buf)
        assert rc == L.QPD_E_UNSUPPORTED and why
    # d_msg off the 8-byte grid with rows of a multiple of 8 bits (K = 64): refused before any launch
    # (include/qpd.h; the generator stores such rows 8 bytes at a time)
    fresh, _ = _float_decoder(env, "SC", N, K)
    for name, buf in (("qpd_mc_llr", llr), ("qpd_mc_decode_f64", out)):
        rc, why = _call(env, name, fresh, ch, None, B, msg.view(-1)[1:], buf)
        assert rc == L.QPD_E_INVALID and "alignment" in why
        assert fresh.info()["last_engine"] == L.QPD_RAN_NONE
    # an empty range: QPD_OK, nothing written (no quantizer needed without rec)
    torch.cuda.synchronize()
    msg.fill_(9), out.fill_(9), llr.fill_(-2.5)
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    bare = L.QpdMcChannel()
    bare.sigma = 0.8
    assert _call(env, "qpd_mc_llr", dec, bare, None, 0, msg, llr)[0] == L.QPD_OK
    assert _call(env, "qpd_mc_decode_f64", dec, bare, None, 0, msg, out, counts)[0] == L.QPD_OK
    torch.cuda.synchronize()
    assert bool((msg == 9).all()) and bool((out == 9).all()) and bool((llr == -2.5).all()) and counts.tolist() == [0, 0]


def test_simulate_on_a_float_decoder(env):
    MC = env.MC
    N, K, L = 128, 64, 8
    dec, _ = _float_decoder(env, "SCL", N, K, L)
    a = MC.simulate(dec, K, [1.0, 3.0, 5.0], batch=3000, max_blocks=20000, stop_blkerrs=200)
    b = MC.simulate(dec, K, [1.0, 3.0, 5.0], batch=777, max_blocks=20000, stop_blkerrs=200)
    for x, y in zip(a, b):
        assert (x.bit_errors, x.block_errors, x.blocks) == (y.bit_errors, y.block_errors, y.blocks)
    assert a[0].bler > a[1].bler > a[2].bler
    quiet = MC.GpuLlrFrames(dec, 1e-3, seed=8)
    msg, bits = quiet.decode_frames(0, 500)
    assert env.torch.equal(msg, bits)


def test_float_and_lut_decoders_get_the_same_frames(env):
    """Paired comparison: one (seed, frame0, B) gives a float SCL handle (qpd_mc_llr) and
    an SCL-LUT handle of the same code (qpd_mc_frames) the same messages, and the LUT
    decoder's symbols are the float decoder's LLRs, quantized."""
    import quantized_decoder_polar_codes_amd as Q
    from quantized_decoder_polar_codes_amd import lut as LU

    N, K, L = 128, 64, 4
    mb, fm, nt = _code(env.C, N, K)
    fdec = env.from_quant("SCL", N, K, fm, L=L)
    ldec = Q.from_packed("SCL-LUT", LU.minsum_uniform_luts(N), K, fm, L=L)
    edges, lut = env.MC.uniform_channel_quantizer(16, 0.5)
    msg_f, llr = env.MC.GpuLlrFrames(fdec, 0.7, seed=2024)(123456, 500)
    msg_l, sym = env.MC.GpuFrames(ldec, edges, lut, 16, 0.7, seed=2024)(123456, 500)
    env.torch.cuda.synchronize()
    assert env.torch.equal(msg_f, msg_l)
    assert np.array_equal(env.C.quantize_channel(llr.cpu().numpy(), edges, lut, 16), sym.cpu().numpy())
