"""The host engine's float paths (SC, SCL, CA-SCL, FastSC, FastSCL) on the
masks and frames of tests/float_cases.py, against the oracle: the decoded
bits through the harness of test_host_engine.py, and for the list kinds the
output path's metric and CRC verdict through the status harness of
test_status_host.py.  The re-quantized kinds are not the host engine's: it
refuses them.
"""
import numpy as np
import pytest

import float_cases as F
from conftest import assert_frames_equal
from test_host_engine import harness, run  # noqa: F401  (harness: the fixture, reused)
from test_status_host import build_status_harness, host_status

QPD_E_UNSUPPORTED = -2
# without the Fast kinds on a labelled root: qpd_create refuses those (qpd_config.hpp: validate, which
# tests/test_capi_host.py and the GPU grid assert) before any engine is planned
HOST_CASES = [c for c in F.cases() if c.kind in F.HOST_KINDS and not c.refused]


@pytest.fixture(scope="module")
def status_harness():
    return build_status_harness()


def host_decoder(c):
    from quantized_decoder_polar_codes_amd.decoders import from_quant

    fm, nt, K = F.code_of(c.N, c.mask)
    return from_quant(c.kind, c.N, K, fm, L=c.L, node_type=nt, quant=F.quant_of(c), create=False, **F.decoder_kw(c))


@pytest.mark.parametrize("c", HOST_CASES, ids=lambda c: c.id)
def test_host_engine_float_grid_matches_oracle(c, harness, status_harness, oracle_mod):  # noqa: F811
    dec = host_decoder(c)
    x = F.frames_of(c)
    assert_frames_equal(run(harness, dec, x), F.reference(c), None, f"host-float-grid-{c.id}")
    if c.kind not in F.LIST_KINDS:
        return
    ca = c.kind == "CA-SCL"
    rows = np.arange(len(x))
    for mb in ((0, 1, F.ca_of(c)[1]) if ca else (0,)):
        bits, pml, winner, passed = F.reference_status(c, mb)
        rc, got, m, ok = host_status(status_harness, dec, x, mask=F.crc_mask(mb) if mb else None, crc_pass=ca)
        assert rc == 0, (c.id, mb)
        assert (got == bits).all(), (c.id, mb)
        assert (m == pml[rows, winner]).all(), (c.id, mb)
        if ca:
            assert (ok == passed).all(), (c.id, mb)


def test_ca_frames_decide_both_ways():
    """The CA-SCL frames of the grid: on every case some frames pass the CRC and some fail, and a one-bit mask
    changes the winner or the verdict of some frame -- the verdict compared above is not a constant."""
    for c in F.cases():
        if c.kind == "CA-SCL":
            a, b = F.reference_status(c, 0), F.reference_status(c, 1)
            assert a[3].any() and not a[3].all(), c.id
            assert ((a[2] != b[2]) | (a[3] != b[3])).any(), c.id


def test_host_engine_refuses_the_requantized_kinds(harness, status_harness):  # noqa: F811
    """No plan is made for them: the decode harness reports that (its -2), the status call QPD_E_UNSUPPORTED."""
    for kind in ("SC-Uniform", "SCL-Uniform", "SC-Lloyd", "SCL-Lloyd"):
        c = next(c for c in F.cases() if c.kind == kind)
        with pytest.raises(ValueError, match="-2"):
            run(harness, host_decoder(c), F.frames_of(c))
        if kind in F.LIST_KINDS:
            rc, _, _, _ = host_status(status_harness, host_decoder(c), F.frames_of(c), crc_pass=False)
            assert rc == QPD_E_UNSUPPORTED, kind
