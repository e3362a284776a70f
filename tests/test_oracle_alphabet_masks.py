"""The CPU oracle against the reference compiled from its own sources, away from the one point the other pins
use (v = 16, a nested reliability order): alphabets of 2 .. 256 symbols and random, block-structured and edge
masks (tests/code_masks.py), tie-heavy tables with one quanta row per element and per node.  This is what lets
the GPU tests of test_gpu_alphabet_masks.py take the oracle as the expected value there.  Skipped, like
test_oracle_vs_reference_random, where the reference build (oracle/_ref) is absent."""
import functools

import numpy as np
import pytest

import code_masks as M
from test_oracle import _ref_decoder

KINDS = ["SC-LUT", "SCL-LUT", "FastSC-LUT", "FastSCL-LUT"]


def list_size(N, v):
    """L of a case: 8, and 3, 4 and 16 in turn, so that a non-power-of-two and a wide list meet the alphabets."""
    return (8, 4, 16, 3)[(N.bit_length() + v) % 4]


@functools.lru_cache(maxsize=2)
def tables(N, v, node_rows):
    """(packed, reference nested lists) of one table set; the grid keeps a set's cases adjacent."""
    from quantized_decoder_polar_codes_amd import lut as LU

    p = LU.random_luts(N, v, seed=11 * N + v + node_rows, distinct_mags=3, node_rows=node_rows)
    return p, LU.unpack_to_reference(p)


def frames(N, v, name, B):
    return np.random.default_rng(N + v + len(name)).integers(0, v, size=(B, N), dtype=np.int32)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("v,N,mask,node_rows", M.cpu_grid(), ids=lambda x: str(x))
def test_oracle_vs_reference_alphabet_masks(v, N, mask, node_rows, kind, oracle_mod):
    R = oracle_mod.reference_module()
    if R is None:
        pytest.skip("reference build (oracle/_ref) not present")
    fm = M.named_mask(N, mask)
    nt = M.node_type_of(fm)
    K, L = int((fm == 0).sum()), list_size(N, v)
    p, (fs, gs, vcl) = tables(N, v, node_rows)
    sym = frames(N, v, mask, 12)
    if M.special_root(fm, kind):  # undefined behaviour in the reference: the oracle refuses
        assert mask == "all_info"
        with pytest.raises(RuntimeError):
            oracle_mod.decode_lut(kind, p, K, L, fm, sym, node_type=nt)
        return
    d = _ref_decoder(R, kind, N, K, L, fm.tolist(), (1 - fm).tolist(), nt.tolist(), fs, gs, vcl)
    ref = np.stack([d.decode(s) for s in sym]).reshape(len(sym), K)
    got = oracle_mod.decode_lut(kind, p, K, L, fm, sym, node_type=nt)
    assert (ref == got).all()


@pytest.mark.parametrize("kind", ["CA-SCL-LUT", "CA-FastSCL-LUT"])
def test_oracle_vs_reference_ca_v8_block_mask(kind, oracle_mod):
    """The CRC-aided kinds at v = 8 on a block mask, on frames that carry a real CRC."""
    R = oracle_mod.reference_module()
    if R is None:
        pytest.skip("reference build (oracle/_ref) not present")
    from quantized_decoder_polar_codes_amd import lut as LU

    N, v, L = 256, 8, 8
    fm = M.block_mask(N, M.BLOCK_SEEDS[N][0])
    nt = M.node_type_of(fm)
    K = int((fm == 0).sum())
    A = K - 24
    p = LU.minsum_uniform_luts(N, v=v)
    fs, gs, vcl = LU.unpack_to_reference(p)
    msg, sym = M.ca_frames(oracle_mod.crc_encode, fm, A, 24, oracle_mod.CRC24_LOC, v, 40, seed=8)
    fz, mm = fm.tolist(), (1 - fm).tolist()
    if kind == "CA-SCL-LUT":
        d = R.CASCLLUTDecoder(N, K, A, L, fz, mm, 24, list(oracle_mod.CRC24_LOC), fs, gs, vcl)
    else:
        d = R.CAFastSCLLUTDecoder(N, K, A, L, fz, mm, nt.tolist(), fs, gs, vcl)
    ref = np.stack([d.decode(s) for s in sym])
    got = oracle_mod.decode_lut_ca(kind, p, K, A, L, fm, sym, node_type=nt)
    assert (ref == got).all()
    ok = (got == msg).all(1).mean()
    assert 0.0 < ok < 1.0, ok  # frames the code corrects and frames it does not: the CRC check goes both ways
