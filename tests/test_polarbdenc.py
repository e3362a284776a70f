"""The drop-in package PolarBDEnc (PolarBDEnc.Encoder.PolarEnc / CRCEnc, the import of every
reference driver that the reference does not ship): CRCEnc, host code, against
oracle.crc_encode; PolarEnc sits on a decoder handle, hence a device -- its cases are marked gpu
and run on the host (qpd_encode_host), frame by frame against codes.polar_encode and the
library's batch call."""
import numpy as np
import pytest

import tx_cases as T


def test_package_has_the_drivers_module_paths():
    import PolarBDEnc
    from PolarBDEnc.Encoder.CRCEnc import CRCEnc
    from PolarBDEnc.Encoder.PolarEnc import PolarEnc

    assert PolarBDEnc.Encoder.PolarEnc.PolarEnc is PolarEnc and PolarBDEnc.Encoder.CRCEnc.CRCEnc is CRCEnc


@pytest.mark.parametrize("crc_n,loc", [(24, T.CRC24_LOC), (11, (11, 10, 9, 5, 0)), (6, (6, 5, 0)), (1, (1, 0))])
@pytest.mark.parametrize("A", (1, 31, 33, 64, 100))
def test_crcenc_matches_the_oracle(crc_n, loc, A):
    import oracle
    from PolarBDEnc.Encoder.CRCEnc import CRCEnc

    enc = CRCEnc(crc_n, list(loc))
    msg = np.random.default_rng(A + crc_n).integers(0, 2, size=(67, A), dtype=np.uint8)
    want = np.concatenate([msg, oracle.crc_encode(msg, crc_n, loc)], axis=1)
    assert (enc.encode_batch(msg) == want).all()
    for f in range(5):  # the drivers' call, frame by frame
        one = enc.encode(msg[f])
        assert one.shape == (A + crc_n,) and one.dtype == np.uint8 and (one == want[f]).all()


def test_crcenc_refuses_coefficients_outside_the_polynomial():
    from PolarBDEnc.Encoder.CRCEnc import CRCEnc

    with pytest.raises(ValueError, match="crc_p"):
        CRCEnc(8, [9, 0])


@pytest.mark.gpu
@pytest.mark.host_engine
@pytest.mark.parametrize("N,name", [(32, "random"), (128, "info0"), (1024, "block5")], ids=lambda v: str(v))
def test_polarenc_agrees_with_polar_encode_frame_by_frame(N, name):
    from PolarBDEnc.Encoder.PolarEnc import PolarEnc
    from quantized_decoder_polar_codes_amd import codes as C

    fm = T.mask_for(N, name)
    mb, fb = np.flatnonzero(fm == 0), np.flatnonzero(fm == 1)
    K = mb.size
    enc = PolarEnc(N, K, fb.tolist(), mb.tolist())
    msg = np.random.default_rng(N).integers(0, 2, size=(12, K), dtype=np.uint8)
    want = C.polar_encode(msg, mb, N)
    for f in range(12):
        one = enc.encode(msg[f])
        assert one.shape == (N,) and (one == want[f]).all()
    assert (enc.encode_batch(msg) == want).all()
    # an index list in another order: message bit i still sits at msgbits[i]
    perm = np.random.default_rng(1).permutation(K)
    shuffled = PolarEnc(N, K, fb.tolist(), mb[perm].tolist())
    assert (shuffled.encode(msg[0]) == C.polar_encode(msg[0], mb[perm], N)).all()
    assert (shuffled.encode_batch(msg) == C.polar_encode(msg, mb[perm], N)).all()


@pytest.mark.gpu
@pytest.mark.host_engine
def test_drivers_chain_crcenc_then_polarenc():
    """mainQuantizedDecoder_LLRDomain.py:153-158 -- and the CRC-aided decoder's own encode_batch gives that word."""
    from PolarBDEnc.Encoder.CRCEnc import CRCEnc
    from PolarBDEnc.Encoder.PolarEnc import PolarEnc
    from quantized_decoder_polar_codes_amd import decoders as D

    fm, msg = T.rnti_case()
    mb = np.flatnonzero(fm == 0)
    crc, pol = CRCEnc(24, list(T.CRC24_LOC)), PolarEnc(T.RNTI_N, mb.size, np.flatnonzero(fm).tolist(), mb.tolist())
    want_info, want_cw = T.encode_ref(fm, msg[:8], A=T.RNTI_A)
    for f in range(8):
        assert (pol.encode(crc.encode(msg[f])) == want_cw[f]).all()
    dec = D.from_quant("CA-SCL", T.RNTI_N, mb.size, fm, L=T.RNTI_L, A=T.RNTI_A, crc_n=24, crc_loc=T.CRC24_LOC)
    info, cw = dec.encode_batch(msg[:8], return_info=True)
    assert (info == want_info).all() and (cw == want_cw).all()
    with pytest.raises(ValueError, match="0 or 1"):
        dec.encode_batch(msg[:8] * 2)
