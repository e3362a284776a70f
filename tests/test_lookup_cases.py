"""The lookup harness's inputs and reference, checked without a GPU.

The generators of tests/lookup_cases.py assert their own coverage -- every (element position,
index, table half) cell of the lookups, every (position, value) cell of the channel readers --
and these tests run them at every alphabet size the GPU tests use, so a generator that stopped
covering its domain fails here.  tests/lookup_ref.py, the numpy reference the device functions
are compared with, is pinned to the reference decoder: an SC-LUT decode built from its f and g
alone must give the oracle's bits.
"""
import numpy as np
import pytest

import lookup_cases as C
import lookup_ref as R


@pytest.mark.parametrize("v", C.LOOKUP_V)
def test_lookup_generators_cover_every_cell(v):
    rng = np.random.default_rng(100 + v)
    for ne in (2, 4, 8):
        for isg in (False, True):
            assert C.vec_case(ne, v, isg, False, rng)["coverage"] == 1.0
    assert C.vec_case(8, v, True, True, rng)["coverage"] == 1.0
    for ne, il, has_h in ((2, False, False), (2, False, True), (4, True, False), (4, True, True)):
        assert C.byte_case(ne, v, has_h, il, rng)["coverage"] == 1.0
    assert C.lut4_case(v, rng)["coverage"] == 1.0


def test_lookup_coverage_assertion_bites():
    rng = np.random.default_rng(1)
    a, b, u = C.lookup_elements(8, 16, 2, rng)
    keep = ~((a[:, 3] == 5) & (b[:, 3] == 9) & (u[:, 3] == 1))  # drop one cell's lanes
    with pytest.raises(AssertionError):
        C.assert_lookup_coverage(a[keep], b[keep], u[keep], 8, 16, 2)


@pytest.mark.parametrize("v", C.CHAN_V)
def test_channel_generators_cover_every_cell(v):
    rng = np.random.default_rng(200 + v)
    for u8 in (False, True):
        for base in (0, 3):
            assert C.chan_case(u8, v, base, rng)["coverage"] == 1.0
        assert C.chan_case(u8, v, 1, rng, counted=True)["coverage"] == 1.0
    c = C.chan_case(False, v, 0, rng)
    cells = 8 * (256 + len(C.I32_EXTRA))  # (the lanes after them pad the last block)
    assert c["err"][:cells].sum() == 8 * (256 - v + len(C.I32_EXTRA))  # exactly the lanes that hold a bad symbol


def test_helper_generators():
    h = C.helper_cases(np.random.default_rng(3))
    assert h["nib_pack4"][0].size == 1 << 16 and h["nib2byte4"][0].size == 1 << 16
    assert h["polar_word"][0].size == 32 + 4096 and h["half_bits4"][0].size == 16
    # polar_word of the reference: an involution, and the unit words give the rows of F^{(x)5}
    x, y = h["polar_word"]
    assert np.array_equal(R.polar_word(y), x)
    assert y[0] == 1 and y[31] == 0xFFFFFFFF and y[1] == 3
    # interleaved order: element k < 4 in the high nibble of byte k, element k + 4 in the low one
    assert R.pack_il(np.arange(1, 9)[None, :])[0] == 0x48372615
    assert np.array_equal(R.unpack_il(R.pack_il(np.arange(8)[None, :]), 8)[0], np.arange(8))
    assert np.array_equal(R.unpack_words(R.pack_words(np.arange(16)[None, :] % 16))[0], np.arange(16))


def test_tables_hold_every_value():
    for v in C.LOOKUP_V:
        tf, tg = C.random_tables(v, np.random.default_rng(v))
        for t in (tf, tg):
            assert len(np.unique(t)) == min(16, 2 * v * v)
    tf, tg = C.index_tables(16)
    assert tf[0, 3, 9] == 9 and tf[1, 3, 9] == 3 and tg[0, 3, 9] == 9 and tg[1, 3, 9] == 3


def test_op_cases_permute_inside_the_groups():
    rng = np.random.default_rng(5)
    tf, tg = C.random_tables(16, rng)
    for kind, isg, cnt, spaces in (("fg", True, 64, 4), ("ff", True, 32, 8), ("gsel", True, 16, 0), ("chan", False, 4, 0)):
        c = C.op_case(kind, isg, cnt, 16, 2, 8, spaces, tf, tg, rng)
        assert c["nonidentity"]
        assert not np.array_equal(c["exp_lds"], c["lds"]) or not np.array_equal(c["exp_slab"], c["slab"])


@pytest.mark.parametrize("N", [16, 64])
@pytest.mark.parametrize("v", [3, 16])
def test_reference_f_g_decode_as_the_oracle(oracle_mod, N, v):
    """SC-LUT from lookup_ref's f and g alone (leaf decision from virtual_channel_llr, construct_pw masks)
    gives oracle.decode_lut("SC-LUT")'s bits on 200 random frames."""
    from quantized_decoder_polar_codes_amd import codes, lut

    K = N // 2
    _, _, fm, _ = codes.construct_pw(N, K)
    p = lut.random_luts(N, v, seed=31 * N + v, distinct_mags=3)
    sym = np.random.default_rng(N + v).integers(0, v, size=(200, N), dtype=np.int32)
    want = oracle_mod.decode_lut("SC-LUT", p, K, 1, fm, sym)
    got = R.sc_lut_decode(p, fm, sym)
    assert got.shape == want.shape
    assert np.array_equal(got, want), f"{int((got != want).any(1).sum())}/200 frames differ"
