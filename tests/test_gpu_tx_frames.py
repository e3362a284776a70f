"""qpd_tx_frames (tx_frames_kernel, csrc/qpd_tx.hip) on the device:

* bit for bit qpd_mc_frames' symbols and qpd_mc_llr's doubles when fed the messages the
  generator drew for the range -- int32 and uint8 symbols, LLRs with and without rec; LUT and
  float kinds, CRC-aided ones; frame ids across 2^32; seeds 1 and 2^64 - 1; a uniform, a
  clustered and a 256-symbol quantizer;
* messages the generator did not draw (all-zero, all-one, fixed random): symbols ==
  codes.quantize_channel of the call's own LLRs, LLRs within 2e-13 / sigma of the
  tests/mc_ref.py restatement for that codeword -- the bound
  tests/test_gpu_mc_llr.py::test_llrs_match_restatement derives for the same arithmetic;
* no_signal: independent of the message (NULL included), the restatement without the BPSK term;
* the RNTI round trip of tests/tx_cases.py on the decode kernels; sub-ranges.
"""
import ctypes

import numpy as np
import pytest

import mc_cases
import tx_cases as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(native_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from quantized_decoder_polar_codes_amd import _lib
    from quantized_decoder_polar_codes_amd import codes as C
    from quantized_decoder_polar_codes_amd import decoders as D
    from quantized_decoder_polar_codes_amd import lut as LU
    from quantized_decoder_polar_codes_amd import montecarlo as MC

    class Env:
        pass

    e = Env()
    e.torch, e.L, e.C, e.D, e.LU, e.MC = torch, _lib, C, D, LU, MC
    e.quant = {k: D.ChannelQuantizer(*mc_cases.quantizers()[k]) for k in ("uniform", "clustered", "q256", "q3")}
    return e


def make_decoder(env, kind, N, K, A=None, v=16):
    _, mb, fm, _ = env.C.construct_pw(N, K)
    if kind in ("SCL-LUT", "CA-SCL-LUT"):
        return env.D.from_packed(kind, env.LU.random_luts(N, v, seed=N + v), K, fm, L=4, **({"A": A} if A else {})), fm
    if kind == "CA-SCL":
        return env.D.from_quant("CA-SCL", N, K, fm, L=4, A=A, crc_n=24, crc_loc=T.CRC24_LOC), fm
    return env.D.from_quant("SC", N, K, fm), fm


# (kind, N, K, A, v, quantizer, frame0, seed)
PARITY = [
    ("SCL-LUT", 128, 64, None, 16, "uniform", 0, 1),
    ("SCL-LUT", 32, 16, None, 8, "q3", 2 ** 32 - 3, 2 ** 64 - 1),  # q < v
    ("SCL-LUT", 1024, 512, None, 16, "clustered", 2 ** 32 - 3, 1),
    ("CA-SCL-LUT", 128, 61, 53, 16, "uniform", 0, 2 ** 64 - 1),  # K - A = 8
    ("CA-SCL-LUT", 128, 64, 40, 16, "q256", 2 ** 32 - 3, 1),  # K - A = 24
    ("CA-SCL-LUT", 1024, 124, 100, 16, "clustered", 0, 1),
    ("SC", 32, 16, None, 16, "q256", 0, 2 ** 64 - 1),
    ("SC", 1024, 512, None, 16, "uniform", 2 ** 32 - 3, 2 ** 64 - 1),
    ("CA-SCL", 128, 64, 40, 16, "clustered", 2 ** 32 - 3, 2 ** 64 - 1),
    ("CA-SCL", 32, 25, 1, 16, "uniform", 0, 1),
]


@pytest.mark.parametrize("kind,N,K,A,v,qname,frame0,seed", PARITY, ids=lambda v: str(v))
def test_generator_messages_give_the_generator_frames(env, kind, N, K, A, v, qname, frame0, seed):
    torch = env.torch
    dec, _ = make_decoder(env, kind, N, K, A, v)
    qz = env.quant[qname]
    B, sigma = 67, env.MC.sigma_for(2.0, K / N)
    msg, sym = env.MC.GpuFrames(dec, qz.edges, qz.lut, qz.q, sigma, seed)(frame0, B)
    assert msg.shape == (B, dec.A)
    got = dec.transmit_batch(msg, sigma, seed, frame0=frame0, quantizer=qz, out="symbols")
    assert got.dtype == torch.int32 and torch.equal(got, sym)
    got8 = dec.transmit_batch(msg, sigma, seed, frame0=frame0, quantizer=qz, out="symbols_u8")
    assert got8.dtype == torch.uint8 and torch.equal(got8.to(torch.int32), sym)
    msg2, llr = env.MC.GpuLlrFrames(dec, sigma, seed)(frame0, B)
    assert torch.equal(msg2, msg)
    mine = dec.transmit_batch(msg, sigma, seed, frame0=frame0)
    assert mine.dtype == torch.float64 and torch.equal(mine.view(torch.int64), llr.view(torch.int64))  # the same doubles
    rec = np.linspace(-7.5, 7.5, qz.q) if qz.q > 3 else np.array([-2.0, 0.25, 3.0])
    _, rllr = env.MC.GpuLlrFrames(dec, sigma, seed, edges=qz.edges, lut=qz.lut, q=qz.q, rec=rec)(frame0, B)
    mine = dec.transmit_batch(msg, sigma, seed, frame0=frame0, quantizer=qz, rec=rec)
    assert torch.equal(mine.view(torch.int64), rllr.view(torch.int64))
    # a zero mask counts as no mask; numpy in -> numpy out, the same symbols
    if A:
        z = dec.transmit_batch(msg, sigma, seed, frame0=frame0, quantizer=qz, out="symbols", crc_mask=np.zeros(16, np.uint8))
        assert torch.equal(z, sym)
    host = dec.transmit_batch(msg.cpu().numpy(), sigma, seed, frame0=frame0, quantizer=qz, out="symbols")
    assert isinstance(host, np.ndarray) and (host == sym.cpu().numpy()).all()
    assert env.L.load().qpd_check_input_error(dec._h) == 0


@pytest.mark.parametrize("kind,N,K,A", [("SC", 128, 64, None), ("CA-SCL", 128, 64, 40), ("SCL-LUT", 1024, 512, None)])
@pytest.mark.parametrize("which", ("zeros", "ones", "random"))
def test_chosen_messages(env, kind, N, K, A, which):
    torch = env.torch
    dec, fm = make_decoder(env, kind, N, K, A)
    B, seed, frame0, sigma = 48, 424242, 5, env.MC.sigma_for(2.0, K / N)
    msg = {"zeros": np.zeros((B, dec.A), np.uint8), "ones": np.ones((B, dec.A), np.uint8),
           "random": np.random.default_rng(77).integers(0, 2, size=(B, dec.A), dtype=np.uint8)}[which]
    mask = T.RNTI_MASK if A else None
    dmsg = torch.from_numpy(msg).cuda()
    llr = dec.transmit_batch(dmsg, sigma, seed, frame0=frame0, crc_mask=mask).cpu().numpy()
    for qname in ("uniform", "clustered"):
        qz = env.quant[qname]
        sym = dec.transmit_batch(dmsg, sigma, seed, frame0=frame0, crc_mask=mask, quantizer=qz, out="symbols").cpu().numpy()
        assert (sym == env.C.quantize_channel(llr, qz.edges, qz.lut, qz.q)).all()
    x = T.encode_ref(fm, msg, A=A, mask=mask)[1]
    if which == "zeros" and not A:
        assert not x.any()  # the all-zero codeword
    err = float(np.abs(llr - T.llr_ref(x, seed, frame0, sigma)).max())
    print(f"max |llr - restatement| = {err:.3e} (bound {2e-13 / sigma:.3e}) {kind} N={N} {which}")
    assert err <= 2e-13 / sigma
    assert (dec.encode_batch(dmsg, crc_mask=mask).cpu().numpy() == x).all()


@pytest.mark.parametrize("kind,N,K,A", [("SC", 128, 64, None), ("CA-SCL-LUT", 128, 64, 40)])
def test_no_signal_is_noise_alone(env, kind, N, K, A):
    torch = env.torch
    dec, _ = make_decoder(env, kind, N, K, A)
    B, seed, frame0, sigma = 48, 2 ** 64 - 1, 2 ** 32 - 3, 0.8
    qz = env.quant["uniform"]
    a = torch.zeros((B, dec.A), dtype=torch.uint8, device="cuda")
    b = torch.ones((B, dec.A), dtype=torch.uint8, device="cuda")
    for out, kw in (("llr", {}), ("symbols", {"quantizer": qz}), ("symbols_u8", {"quantizer": qz})):
        ra = dec.transmit_batch(a, sigma, seed, frame0=frame0, signal=False, out=out, **kw)
        rb = dec.transmit_batch(b, sigma, seed, frame0=frame0, signal=False, out=out, **kw)
        rn = dec.transmit_batch(B, sigma, seed, frame0=frame0, signal=False, out=out, **kw)  # d_msg = NULL
        rn = torch.from_numpy(rn).cuda()
        assert torch.equal(ra, rb) and torch.equal(ra, rn)
        if out == "llr":
            llr = ra.cpu().numpy()
        else:
            assert (ra.cpu().numpy() == env.C.quantize_channel(llr, qz.edges, qz.lut, qz.q)).all()
    err = float(np.abs(llr - T.llr_ref(np.zeros((B, N), np.uint8), seed, frame0, sigma, signal=False)).max())
    print(f"no_signal: max |llr - restatement| = {err:.3e} (bound {2e-13 / sigma:.3e})")
    assert err <= 2e-13 / sigma
    with_signal = dec.transmit_batch(a, sigma, seed, frame0=frame0).cpu().numpy()
    assert np.abs(with_signal - llr).min() > 1.0  # the BPSK term is 2 / sigma^2 in the LLR


@pytest.mark.parametrize("kind,engine", [("CA-SCL-LUT", "fast"), ("CA-SCL", "generic")])
def test_rnti_round_trip_on_the_kernels(env, kind, engine):
    """The committed case of tests/tx_cases.py (confirmed on the host engine in test_encode_host.py)."""
    torch = env.torch
    fm, msg = T.rnti_case()
    N, K = T.RNTI_N, T.RNTI_A + 24
    if kind == "CA-SCL-LUT":
        # min-sum tables: +-20 LLRs are the outermost symbols, and the decode is the float decoder's on them
        from conftest import GOLDEN_DIR, golden_packed, load_golden
        import os

        g = load_golden(os.path.join(GOLDEN_DIR, "ca_scllut_n128_a40_l8_minsum.npz"))
        assert int(g["N"]) == N and int(g["K"]) == K
        fm = np.asarray(g["frozen"], dtype=np.int32)
        dec = env.D.from_packed(kind, golden_packed(g), K, fm, L=T.RNTI_L, A=T.RNTI_A, engine=engine)
        cw = dec.encode_batch(torch.from_numpy(msg).cuda(), crc_mask=T.RNTI_MASK)
        v = int(g["v"])
        x = torch.where(cw == 0, v - 1, 0).to(torch.int32)
    else:
        dec = env.D.from_quant(kind, N, K, fm, L=T.RNTI_L, A=T.RNTI_A, crc_n=24, crc_loc=T.CRC24_LOC, engine=engine)
        cw = dec.encode_batch(torch.from_numpy(msg).cuda(), crc_mask=T.RNTI_MASK)
        x = torch.where(cw == 0, 20.0, -20.0).to(torch.float64)
    bits, st = dec.decode_batch(x, return_status=True, crc_mask=T.RNTI_MASK)
    assert dec.info()["last_engine"] == env.L.QPD_RAN_GPU
    assert bool(st.crc_pass.all()) and (bits.cpu().numpy() == msg).all()
    _, st = dec.decode_batch(x, return_status=True, crc_mask=T.RNTI_OTHER)
    assert dec.info()["last_engine"] == env.L.QPD_RAN_GPU
    assert not bool(st.crc_pass.any())


def test_sub_range_equals_rows_of_the_whole(env):
    torch = env.torch
    dec, _ = make_decoder(env, "CA-SCL", 128, 64, 40)
    B, a, b = 200, 37, 151
    msg = torch.from_numpy(np.random.default_rng(4).integers(0, 2, size=(B, 40), dtype=np.uint8)).cuda()
    qz = env.quant["uniform"]
    for out, kw in (("llr", {}), ("symbols", {"quantizer": qz})):
        whole = dec.transmit_batch(msg, 0.7, 99, frame0=2 ** 32 - 100, crc_mask=T.RNTI_MASK, out=out, **kw)
        part = dec.transmit_batch(msg[a:b], 0.7, 99, frame0=2 ** 32 - 100 + a, crc_mask=T.RNTI_MASK, out=out, **kw)
        assert torch.equal(part, whole[a:b])
    tx = env.MC.GpuTxFrames(dec, 0.7, 99, crc_mask=T.RNTI_MASK)
    m, frames = tx(2 ** 32 - 100 + a, msg[a:b])  # the generate slot's shape: (msg, frames)
    whole = dec.transmit_batch(msg, 0.7, 99, frame0=2 ** 32 - 100, crc_mask=T.RNTI_MASK)
    assert m is msg[a:b] or torch.equal(m, msg[a:b])
    assert torch.equal(frames, whole[a:b])


def test_refusals_and_layout(env):
    torch, lib = env.torch, env.L.load()
    dec, _ = make_decoder(env, "SC", 128, 64)
    qz = env.quant["uniform"]
    msg = torch.zeros((5, 64), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="rec"):
        dec.transmit_batch(msg, 1.0, 1, quantizer=qz, out="symbols", rec=np.zeros(16))
    with pytest.raises(ValueError, match="crc_mask"):
        dec.transmit_batch(msg, 1.0, 1, crc_mask=[1])
    ch = env.L.QpdMcChannel()
    ch.sigma, ch.q, ch.n_edges, ch.edges, ch.lut = 1.0, qz.q, qz.edges.size, qz.edges.ctypes.data, qz.lut.ctypes.data
    rec = np.zeros(16)
    raw = torch.full((5 * 128 + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = lib.qpd_tx_frames(dec._h, ctypes.byref(ch), ctypes.c_void_p(rec.ctypes.data), ctypes.c_uint64(1), 0, 5,
                           ctypes.c_void_p(msg.data_ptr()), None, env.L.QPD_TX_SYM_U8, ctypes.c_void_p(raw.data_ptr()), None)
    assert rc == env.L.QPD_E_INVALID and b"rec" in lib.qpd_last_error()
    # uint8 symbols from an odd base, sentinels around the rows
    want = dec.transmit_batch(msg, 1.0, 1, quantizer=qz, out="symbols_u8")
    rc = lib.qpd_tx_frames(dec._h, ctypes.byref(ch), None, ctypes.c_uint64(1), 0, 5, ctypes.c_void_p(msg.data_ptr()), None,
                           env.L.QPD_TX_SYM_U8, ctypes.c_void_p(raw.data_ptr() + 31),
                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.qpd_last_error()
    torch.cuda.synchronize()
    got = raw.cpu().numpy()
    assert (got[31: 31 + 5 * 128].reshape(5, 128) == want.cpu().numpy()).all()
    assert (got[:31] == 0xA5).all() and (got[31 + 5 * 128:] == 0xA5).all()
