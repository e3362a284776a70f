"""Decode status on the kernels against the CPU oracle, on every status
instantiation: one qpd_decode_status call per case and CRC mask of
tests/status_cases.py, outputs pre-filled with canaries, then

* the bits, the metric (== on float64: the decoder's own PML double of the
  output path) and the verdict are the oracle's (pinned on the CPU by
  tests/test_oracle_status.py; for FastSCL-LUT, CA-FastSCL-LUT, L > 8 and
  float SCL / FastSCL that rests on the oracle and the host engine agreeing, not
  on a recorded reference value; for SCL-Uniform and SCL-Lloyd, which the host
  engine does not decode, on the oracle alone);
* frames past B keep their canaries (partial waves, several launches per call,
  grid-stride rounds);
* the decoder reports the engine, lane groups, frames per wave, kernel variant
  and prefix split the case was written for (status_cases.EXPECT), so a planner
  change cannot move a case onto another kernel unnoticed.
"""
import numpy as np
import pytest

import status_cases as S
from conftest import assert_engine
from test_gpu_status import dev_status, np3

pytestmark = pytest.mark.gpu
PAD = 5  # canary frames after frame B


@pytest.fixture(scope="module")
def qpd(native_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import quantized_decoder_polar_codes_amd as Q

    return Q


def decoder_of(c):
    from quantized_decoder_polar_codes_amd import decoders as D

    fm, nt, _ = S.code_of(c)
    kw = dict(A=c.A, crc_n=c.crc_n, crc_loc=c.crc_loc) if c.A else {}
    if c.max_waves:
        kw["max_waves"] = c.max_waves
    if c.is_float:
        return D.from_quant(c.kind, c.N, c.K, fm, L=c.L, node_type=nt, quant=S.quant_of(c), **kw)
    return D.from_packed(c.kind, S.tables_of(c), c.K, fm, L=c.L, node_type=nt, engine=c.engine, **kw)


@pytest.mark.parametrize("c", S.CASES, ids=lambda c: c.id)
def test_status_matches_oracle(c, qpd, monkeypatch):
    import torch

    for name in S.SWITCH_ENV:
        monkeypatch.delenv(name, raising=False)
    for name, value in c.env:
        monkeypatch.setenv(name, value)
    x, ref = S.reference(c)
    if c.B >= 16:
        S.check_informative(c)
    dec = decoder_of(c)
    info = dec.info()
    got_info = (info["engine"], info["lanes_per_frame"], info["frames_per_wave"], info["fast_variant"], info["prefix_ops"] > 0)
    assert got_info == S.EXPECT[c.id]
    dev = torch.from_numpy(np.ascontiguousarray(x.astype(np.uint8) if c.dtype == "u8" else x)).cuda()
    rows = np.arange(c.B)
    for mb, (bits, pml, winner, passed) in ref.items():
        got, m, ok = np3(dev_status(dec, dev, mask=S.crc_mask(mb) if mb else None, crc_pass=bool(c.A), B=c.B, size=c.B + PAD))
        assert_engine(dec, "gpu")
        assert (got[: c.B] == bits).all(), f"mask {mb}: bits of {(got[: c.B] != bits).any(1).sum()} frames differ"
        bad = np.flatnonzero(m[: c.B] != pml[rows, winner])
        assert bad.size == 0, f"mask {mb}: metric of {bad.size} frames differs, first {bad[:4]}: {m[bad[:4]]} != {pml[bad[:4], winner[bad[:4]]]}"
        if c.A:
            assert (ok[: c.B] == passed).all(), f"mask {mb}: verdict"
        assert (got[c.B:] == 0xEE).all() and (m[c.B:] == -7.0).all() and (ok[c.B:] == 0x55).all(), "frames past B written"
