"""qpd_encode on the device (tx_encode_kernel, csrc/qpd_tx.hip) against the host variant
(qpd_encode_host, itself checked against codes.polar_encode and oracle.crc_encode in
tests/test_encode_host.py): information bits and codewords, byte for byte --

* N = 32 .. 4096, kinds with and without CRC, masks of 0 .. 24 bits, B = 1, 67 and 5000
  (more frames than one resident round of workgroups: the waves stride);
* tensors sliced to odd byte offsets on the input and on both outputs (the byte paths),
  with sentinels around the outputs;
* bad message bytes reported through qpd_check_input_error, the rest of the batch equal.
"""
import ctypes

import numpy as np
import pytest

import tx_cases as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(native_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from quantized_decoder_polar_codes_amd import _lib
    from quantized_decoder_polar_codes_amd import decoders as D

    class Env:
        pass

    e = Env()
    e.torch, e.L, e.D = torch, _lib, D
    return e


def decoder(env, fm, A=None, kind=None):
    fm = np.asarray(fm, dtype=np.int32)
    K = int((fm == 0).sum())
    if A is None:
        return env.D.from_quant(kind or "SC", fm.size, K, fm)
    return env.D.from_quant("CA-SCL", fm.size, K, fm, L=4, A=A, crc_n=24, crc_loc=T.CRC24_LOC)


# (N, mask name, K, A, mask bits, B)
CASES = [(32, "random", 16, None, 0, 1), (32, "all_info", None, None, 0, 67), (32, "random", 20, None, 0, 5000),
         (128, "info0", None, None, 0, 67), (128, "random", 64 + 24, 64, 16, 67), (128, "random", 31 + 24, 31, 1, 1),
         (1024, "block5", None, None, 0, 67), (1024, "random", 100 + 24, 100, 24, 67), (1024, "alt10", None, None, 0, 1),
         (4096, "random", 2072, None, 0, 67), (4096, "random", 33 + 24, 33, 16, 67), (32, "random", 1 + 24, 1, 24, 5000),
         (32, "random", 20, None, 0, 20011)]  # beyond 32 waves on each of 256 CUs, whatever the occupancy


@pytest.mark.parametrize("N,name,K,A,bits,B", CASES, ids=lambda v: str(v))
def test_device_encoder_equals_host_variant(env, N, name, K, A, bits, B):
    torch = env.torch
    fm = T.mask_for(N, name, K)
    dec = decoder(env, fm, A)
    msg = np.random.default_rng(N + B + bits).integers(0, 2, size=(B, dec.A), dtype=np.uint8)
    mask = None if not bits else np.resize(T.RNTI_MASK, bits)
    want_info, want_cw = dec.encode_batch(msg, crc_mask=mask, return_info=True)  # numpy: qpd_encode_host
    ref_info, ref_cw = T.encode_ref(fm, msg, A=A, mask=mask)
    assert (want_info == ref_info).all() and (want_cw == ref_cw).all()
    info, cw = dec.encode_batch(torch.from_numpy(msg).cuda(), crc_mask=mask, return_info=True)
    assert info.is_cuda and cw.is_cuda and cw.shape == (B, N) and info.shape == (B, dec.K)
    assert (info.cpu().numpy() == want_info).all()
    assert (cw.cpu().numpy() == want_cw).all()
    assert env.L.load().qpd_check_input_error(dec._h) == 0
    # the codeword alone
    assert (dec.encode_batch(torch.from_numpy(msg).cuda(), crc_mask=mask).cpu().numpy() == want_cw).all()


@pytest.mark.parametrize("N,K,A", [(32, 16, None), (128, 88, 64), (1024, 512, None)])
@pytest.mark.parametrize("off_in,off_info,off_cw", [(1, 0, 0), (0, 3, 5), (7, 1, 8), (8, 8, 8)])
def test_odd_byte_offsets_and_sentinels(env, N, K, A, off_in, off_info, off_cw):
    """Slices of byte tensors: every path by alignment, nothing outside the B rows written."""
    torch, lib = env.torch, env.L.load()
    fm = T.mask_for(N, "random", K)
    dec = decoder(env, fm, A)
    B, pad = 67, 64
    msg = np.random.default_rng(off_in + N).integers(0, 2, size=(B, dec.A), dtype=np.uint8)
    want_info, want_cw = dec.encode_batch(msg, return_info=True)
    raw_in = torch.zeros(B * dec.A + 16, dtype=torch.uint8, device="cuda")
    raw_in[off_in: off_in + B * dec.A] = torch.from_numpy(msg.reshape(-1)).cuda()
    raw_info = torch.full((B * dec.K + 2 * pad + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    raw_cw = torch.full((B * N + 2 * pad + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    assert raw_in.data_ptr() % 8 == 0 and raw_info.data_ptr() % 8 == 0 and raw_cw.data_ptr() % 8 == 0
    p_in = raw_in.data_ptr() + off_in
    p_info, p_cw = raw_info.data_ptr() + pad + off_info, raw_cw.data_ptr() + pad + off_cw
    stream = torch.cuda.current_stream().cuda_stream
    rc = lib.qpd_encode(dec._h, ctypes.c_void_p(p_in), B, None, ctypes.c_void_p(p_info), ctypes.c_void_p(p_cw),
                        ctypes.c_void_p(stream))
    assert rc == 0, lib.qpd_last_error()
    torch.cuda.synchronize()
    got_info, got_cw = raw_info.cpu().numpy(), raw_cw.cpu().numpy()
    a, b = pad + off_info, pad + off_cw
    assert (got_info[a: a + B * dec.K].reshape(B, dec.K) == want_info).all()
    assert (got_cw[b: b + B * N].reshape(B, N) == want_cw).all()
    assert (got_info[:a] == 0xA5).all() and (got_info[a + B * dec.K:] == 0xA5).all()
    assert (got_cw[:b] == 0xA5).all() and (got_cw[b + B * N:] == 0xA5).all()


@pytest.mark.parametrize("N,K,A", [(128, 64, None), (128, 57, 33)])
def test_bad_bytes_raise_the_error_word(env, N, K, A):
    torch, lib = env.torch, env.L.load()
    fm = T.mask_for(N, "random", K)
    dec = decoder(env, fm, A)
    msg = np.random.default_rng(9).integers(0, 2, size=(67, dec.A), dtype=np.uint8)
    clean = dec.encode_batch(torch.from_numpy(msg).cuda()).cpu().numpy()
    assert lib.qpd_check_input_error(dec._h) == 0
    for bad, at in ((2, (5, 3)), (255, (66, dec.A - 1))):
        m = msg.copy()
        m[at] = bad
        got = dec.encode_batch(torch.from_numpy(m).cuda()).cpu().numpy()
        assert lib.qpd_check_input_error(dec._h) == env.L.QPD_E_INPUT
        assert b"0 or 1" in lib.qpd_last_error()
        assert lib.qpd_check_input_error(dec._h) == 0  # reported once
        others = np.arange(67) != at[0]
        assert (got[others] == clean[others]).all()
        assert (got[at[0]] == T.encode_ref(fm, m[at[0]: at[0] + 1], A=A)[1][0]).all()  # the low bit counts
        with pytest.raises(ValueError, match="0 or 1"):  # the host variant returns QPD_E_INPUT
            dec.encode_batch(m)


def test_refusals_reach_the_entry_point(env):
    torch, lib = env.torch, env.L.load()
    dec = decoder(env, T.mask_for(128, "random", 64))
    msg = torch.zeros((2, 64), dtype=torch.uint8, device="cuda")
    rc = lib.qpd_encode(dec._h, ctypes.c_void_p(msg.data_ptr()), 2, None, None, None, None)
    assert rc == env.L.QPD_E_INVALID and b"d_codeword" in lib.qpd_last_error()
    with pytest.raises(ValueError, match="crc_mask"):
        dec.encode_batch(msg, crc_mask=[1, 0])
