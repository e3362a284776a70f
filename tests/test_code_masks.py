"""The mask generators of tests/code_masks.py give what the parity tests choose them for (CPU only)."""
import numpy as np
import pytest

import code_masks as M

FAST_KINDS = ("FastSC-LUT", "FastSCL-LUT")


def _block_masks():
    return [M.block_mask(N, s) for N, seeds in M.BLOCK_SEEDS.items() for s in seeds]


def test_generators_are_deterministic_and_well_formed():
    for N in (16, 64, 256):
        for fm in (M.random_mask(N, N // 2, 3), M.block_mask(N, 3), *M.edge_masks(N).values()):
            assert fm.shape == (N,) and fm.dtype == np.int64 and set(np.unique(fm)) <= {0, 1}
        assert np.array_equal(M.block_mask(N, 5), M.block_mask(N, 5))
        assert not np.array_equal(M.block_mask(N, 5), M.block_mask(N, 6))
        assert np.array_equal(M.random_mask(N, N // 4, 5), M.random_mask(N, N // 4, 5))
        assert int((M.random_mask(N, N // 4, 5) == 0).sum()) == N // 4


def test_edge_masks_are_what_their_names_say():
    for N in (16, 256):
        e = M.edge_masks(N)
        assert set(e) == {"info0", "frozen_last", "K1_mid", "KN-1_mid", "all_info", "alt10", "alt01", "antipolar"}
        assert e["info0"][0] == 0 and 1 < int((e["info0"] == 0).sum()) < N // 2
        assert e["frozen_last"][N - 1] == 1 and int(e["frozen_last"].sum()) == 2
        assert np.flatnonzero(e["K1_mid"] == 0).tolist() == [N // 2 + 1]
        assert np.flatnonzero(e["KN-1_mid"] == 1).tolist() == [N // 2 - 1]
        assert not e["all_info"].any()
        assert e["alt10"][:4].tolist() == [1, 0, 1, 0] and e["alt01"][:4].tolist() == [0, 1, 0, 1]
        assert not e["antipolar"][: N // 2].any() and e["antipolar"][N // 2:].all()
        assert M.labelled_nodes(e["antipolar"]) == [("R1", N // 2), ("R0", N // 2)]
        # all_info is the one mask the Fast kinds refuse; every other root is unlabelled
        for name, fm in e.items():
            for kind in FAST_KINDS:
                assert M.special_root(fm, kind) == (name == "all_info"), (N, name, kind)


def test_block_seeds_cover_every_special_node():
    seen = set()
    for fm in _block_masks():
        seen |= set(M.labelled_nodes(fm))
    want = {(t, s) for t in ("R0", "R1", "REP") for s in (2, 4, 8, 16, 32)} | {("SPC", s) for s in (4, 8, 16, 32)}
    assert not want - seen, sorted(want - seen)
    assert ("R1", 32) in seen and ("R1", 64) in seen  # the 17..32 and the > 32 argsort paths of FastSCL-LUT


def test_the_switch_case_has_a_64_element_r1_node():
    assert ("R1", 64) in M.labelled_nodes(M.block_mask(256, M.BLOCK_SEEDS[256][0]))


def test_block_seeds_have_an_r1_node_followed_by_an_r0_node():
    for N, seeds in M.BLOCK_SEEDS.items():
        hit = 0
        for s in seeds:
            ln = M.labelled_nodes(M.block_mask(N, s))
            hit += any(a[0] == "R1" and b[0] == "R0" and a[1] > 1 and b[1] > 1 for a, b in zip(ln, ln[1:]))
        assert hit, N


def test_block_seeds_reach_the_ends_of_the_mask():
    """Position 0 information and position N-1 frozen, which no nested order has, each in some block mask."""
    ms = _block_masks()
    assert any(fm[0] == 0 for fm in ms) and any(fm[-1] == 1 for fm in ms)


@pytest.mark.parametrize("kind", FAST_KINDS)
def test_no_chosen_seed_has_a_special_root(kind):
    """The Fast kinds refuse a labelled root on both sides, and a refused case tests nothing."""
    for fm in _block_masks():
        assert not M.special_root(fm, kind)
    for N, K, seed in M.RANDOM_CASES:
        fm = M.random_mask(N, K, seed)
        assert int((fm == 0).sum()) == K and not M.special_root(fm, kind)
