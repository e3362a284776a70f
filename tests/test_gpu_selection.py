"""The list decoders' 2L -> L survivor selection, called directly on the device.

Every list decoder decides its bits in one place: the selection of the L survivors among
the 2L candidates [keeps | flips], which must be mink's (SCLLUTDecoder.cpp:8-21):
std::sort on the candidate indices by key, first L outputs, libstdc++'s unstable tie
order included once 2L > 16.  A decode reaches only the selection
states its tables and frames happen to produce; the harness (tests/native/sel_harness.hip)
hands chosen keys to the primitives themselves -- select_survivors16 with its parallel
introsort replay and its serial depth-limit fallback, the identity shortcuts keep_all8 /
keep_all16, select_survivors8 and the generic select_survivors -- in the LDS layout of
lut_fast_kernel, between canary words, with each of a wave's four lane groups and each
frame set on keys of its own class, so that the groups differ in partition count and in
whether they are live.

All comparisons are exact, on (parent, upper) of the lanes gl < L, against the harness
library's host reference (std::sort itself); every case also asserts the canaries.
"""
import functools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

INF = np.inf
TINY = np.array([0.0, 5e-324, 1e-310, 2.2250738585072014e-308, 1.0])  # +0, subnormals, the least normal
BLOCKS = 512  # one-wave blocks per launch: 2048 lane groups of 16 per frame set
N_CLASSES = 11


@pytest.fixture(scope="module")
def harness(native_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import sel_harness

    return sel_harness.load()  # rebuilt only when the harness or csrc/ changed


@functools.lru_cache(maxsize=None)
def _witnesses():
    with open(os.path.join(GOLDEN_DIR, "w16_fallback_witnesses.json")) as fh:
        return {int(L): [np.array(k, np.float64) for k in ks] for L, ks in json.load(fh).items()}


def _emulator_mode(rng, L, mode):
    """The six key modes of tests/native/w16_replay_check.cpp: keeps, then flips = keep + penalty."""
    nv = 1 + int(rng.integers(5))
    j = np.arange(L)
    if mode == 0:  # few distinct values, any order
        k = rng.integers(nv, size=L).astype(np.float64)
    elif mode == 1:  # ascending keeps with runs
        k = (j // rng.integers(1, 4, size=L)).astype(np.float64)
    elif mode == 2:  # dead (+inf) paths
        k = np.where(j < rng.integers(L, size=L), rng.integers(3, size=L).astype(np.float64), INF)
    elif mode == 3:  # all equal
        k = np.full(L, 7.0)
    elif mode == 4:  # mixed
        k = np.where((j * 7919) % 11 < 4, j % 3, 10 + j).astype(np.float64)
    else:  # dyadic
        k = np.ldexp(rng.integers(8, size=L).astype(np.float64), -rng.integers(3, size=L))
    pen = np.where((rng.integers(4, size=L) == 0) | (mode == 3), 0.0, 1.0 + rng.integers(nv, size=L))
    return np.concatenate([k, k + pen])


def _group_keys(rng, L, cls, adversary):
    """2L keys of one lane group (keep i at i, flip i at L + i), by class."""
    n2 = 2 * L
    if cls < 6:
        return _emulator_mode(rng, L, cls)
    if cls == 6:  # exact +0 and subnormal keys
        return rng.choice(TINY, size=n2)
    if cls == 7:  # strictly increasing, tie-free: the identity
        return np.cumsum(rng.integers(1, 4, size=n2)).astype(np.float64)
    if cls == 8:  # tie-free, any order
        return rng.permutation(n2).astype(np.float64) + 0.5
    if cls == 9:  # McIlroy's adversary against std::sort of 2L elements, sometimes one entry changed
        k = adversary[n2].copy()
        if rng.integers(2):
            k[rng.integers(n2)] = float(rng.integers(n2))
        return k
    # deep partitions: the committed depth-limit witnesses of this L and their single-entry
    # mutations; an L without a witness takes a resized one (deep, short of the limit)
    wit = _witnesses()
    if L in wit:
        k = wit[L][int(rng.integers(len(wit[L])))].copy()
    else:
        base = wit[15][int(rng.integers(len(wit[15])))]
        k = base[:n2].copy() if n2 <= base.size else np.concatenate([base, rng.integers(16, size=n2 - base.size)])
    if rng.integers(3) == 0:
        k[rng.integers(n2)] = float(rng.integers(16))
    return k


_CACHE = {}


def _w16_case(harness, L, nsets):
    """Keys of BLOCKS waves x nsets sets x 4 groups of 16 (every class in every group
    position), with the host's reference selection and depth-limit predicate: computed
    once and shared by the tests."""
    if (L, nsets) in _CACHE:
        return _CACHE[L, nsets]
    rng = np.random.default_rng(1000 * L + nsets)
    adversary = {2 * L: harness.adversary(2 * L)}
    keep = np.empty((BLOCKS, nsets, 64))
    flip = np.empty((BLOCKS, nsets, 64))
    cls = rng.integers(N_CLASSES, size=(BLOCKS, nsets, 4))
    cls[:N_CLASSES, :, :] = (np.arange(N_CLASSES)[:, None, None] + np.arange(4)[None, None, :]) % N_CLASSES
    for b in range(BLOCKS):
        for s in range(nsets):
            for g in range(4):
                k = _group_keys(rng, L, int(cls[b, s, g]), adversary)
                lanes = slice(16 * g, 16 * g + L)
                # the padding lanes gl >= L carry junk: the primitives must treat them as +inf
                keep[b, s, 16 * g: 16 * g + 16] = rng.choice([0.0, 1.0, INF], size=16)
                flip[b, s, 16 * g: 16 * g + 16] = rng.choice([0.0, 1.0, INF], size=16)
                keep[b, s, lanes] = k[:L]
                flip[b, s, lanes] = k[L:]
    want = harness.reference(L, 16, keep, flip)
    fell, parts = harness.fallback(L, keep, flip)
    keep.setflags(write=False)
    flip.setflags(write=False)
    _CACHE[L, nsets] = (keep, flip, cls, want, fell, parts)
    return _CACHE[L, nsets]


def _assert_selection(got_parent, got_upper, want, L, gs, label):
    live = (np.arange(64) % gs) < L
    wp, wu = want
    bad = ((got_parent != wp) | (got_upper != wu))[..., live]
    if bad.any():
        b, s, _ = np.argwhere(bad)[0]
        g = int(np.flatnonzero(bad[b, s])[0]) // L * gs
        pytest.fail(f"{label}: {int(bad.any(-1).sum())} waves differ from std::sort; first: block {b} set {s} group at lane {g}\n"
                    f" got  parent {got_parent[b, s, g:g + L].tolist()} upper {got_upper[b, s, g:g + L].tolist()}\n"
                    f" want parent {wp[b, s, g:g + L].tolist()} upper {wu[b, s, g:g + L].tolist()}")


def test_reference_is_argsort_on_tie_free_keys(harness):
    """The reference itself: without ties every correct sort agrees, so mink's first L
    outputs are numpy.argsort's."""
    rng = np.random.default_rng(5)
    for L, gs in ((3, 4), (8, 8), (13, 16), (16, 16)):
        keys = np.stack([rng.permutation(2 * L).astype(np.float64) for _ in range(64 // gs * 8)])  # [groups, 2L]
        keep = np.full((8, 64 // gs, gs), INF)
        flip = np.full((8, 64 // gs, gs), INF)
        keep[..., :L] = keys[:, :L].reshape(8, -1, L)
        flip[..., :L] = keys[:, L:].reshape(8, -1, L)
        parent, upper = harness.reference(L, gs, keep.reshape(8, 64), flip.reshape(8, 64))
        order = np.argsort(keys, axis=1, kind="stable")[:, :L].reshape(8, -1, L)
        assert np.array_equal(parent.reshape(8, -1, gs)[..., :L], order % L)
        assert np.array_equal(upper.reshape(8, -1, gs)[..., :L], order // L)
        assert (parent.reshape(8, -1, gs)[..., L:] == -1).all()


def test_entry_point_refuses_what_the_kernels_cannot_run(harness):
    """L, primitive and set count are validated before anything is launched."""
    import sel_harness as S

    z = np.zeros(2 * 64)
    for prim, L, nsets in ((S.SEL16, 8, 1), (S.SEL16, 17, 1), (S.SEL8, 7, 1), (S.GENERIC, 0, 1), (S.GENERIC, 9, 1),
                           (S.KEEP8, 9, 1), (S.KEEP16, 8, 1), (6, 8, 1), (-1, 8, 1), (S.SEL16, 16, 3), (S.SEL16, 16, 0)):
        assert harness.run_raw(prim, L, nsets, 1, z, z) == -1, (prim, L, nsets)
    assert harness.run_raw(S.SEL16_SERIAL, 16, 1, 1, z, z) == -1  # no group masks
    assert harness.run_raw(S.SEL16_SERIAL, 16, 1, 1, z, z, np.array([16], np.uint8)) == -1  # a fifth group
    assert harness.run_raw(S.SEL16, 16, 1, 0, z, z) == -1


@pytest.mark.parametrize("nsets", [1, 2])
@pytest.mark.parametrize("L", range(9, 17))
def test_select_survivors16(L, nsets, harness):
    """The parallel replay beside groups that stop early, run on, or fall back: 2048
    groups per set, every key class in every group position.  At L = 15 (and wherever
    tests/golden/w16_fallback_witnesses.json holds a witness) some groups take the serial
    depth-limit fallback on their own -- counted on the host by the emulator's predicate."""
    import sel_harness as S

    keep, flip, cls, want, fell, parts = _w16_case(harness, L, nsets)
    assert keep.shape[0] * nsets * 4 >= 2000
    assert all((cls == c).any(axis=(0, 1)).all() for c in range(N_CLASSES))  # every class in every group position
    print(f"L={L} sets={nsets}: natural fallbacks {int(fell.sum())}, partitions per group up to {int(parts.max())}, "
          f"waves with differing trip counts {int((parts.max(-1) != parts.min(-1)).any(-1).sum())}")
    assert 15 in _witnesses()
    if L in _witnesses():  # L = 15 always; any other L the checker's search found a witness for
        assert fell.sum() >= 1, "no group took the natural depth-limit fallback"
        assert (fell.any(-1) & ~fell.all(-1)).any(), "no wave with a fallback group beside a live one"
    assert (parts.max(-1) != parts.min(-1)).any()  # the four groups of a wave differ in trip count
    parent, upper, _, canary = harness.run(S.SEL16, L, keep, flip)
    assert canary.all(), f"LDS canaries overwritten in blocks {np.flatnonzero(canary == 0)[:8]}"
    _assert_selection(parent, upper, want, L, 16, f"select_survivors16 L={L} sets={nsets}")


@pytest.mark.parametrize("nsets", [1, 2])
@pytest.mark.parametrize("L", range(9, 17))
def test_select_survivors16_forced_serial(L, nsets, harness):
    """The serial fallback's LDS aliasing (keys as doubles over the set's whole 64-slot
    row, the index array in the junk row, c replaced group after group) next to live
    groups: the same inputs under all 16 group masks; forced and unforced groups alike
    equal the reference."""
    import sel_harness as S

    keep, flip, cls, want, fell, parts = _w16_case(harness, L, nsets)
    force = ((np.arange(BLOCKS)[:, None] + 5 * np.arange(nsets)[None, :]) % 16).astype(np.uint8)
    assert all((force == m).any() for m in range(16))
    bits = (force[..., None] >> np.arange(4)) & 1
    assert bits.sum() > 0 and (1 - bits).sum() > 0
    # forced groups beside groups that run the parallel replay to a natural end or fallback
    assert ((bits == 1).any(-1) & ((bits == 0) & (parts > 0)).any(-1)).any()
    parent, upper, _, canary = harness.run(S.SEL16_SERIAL, L, keep, flip, force)
    assert canary.all(), f"LDS canaries overwritten in blocks {np.flatnonzero(canary == 0)[:8]}"
    _assert_selection(parent, upper, want, L, 16, f"select_survivors16<serial> L={L} sets={nsets}")
    # mask 0 everywhere is the production path: the diagnostic instantiation agrees with it
    p0, u0, _, c0 = harness.run(S.SEL16_SERIAL, L, keep[:64], flip[:64], np.zeros((64, nsets), np.uint8))
    assert c0.all()
    _assert_selection(p0, u0, (want[0][:64], want[1][:64]), L, 16, f"select_survivors16<serial, mask 0> L={L}")


def _identity_waves(rng, L, gs, nb, nsets):
    """Every group: strictly increasing keeps, every flip strictly above the largest keep --
    some keeps one ulp apart, some flips one ulp above the largest keep."""
    keep = np.empty((nb, nsets, 64))
    flip = np.empty((nb, nsets, 64))
    for b in range(nb):
        for s in range(nsets):
            for g in range(0, 64, gs):
                # as bit patterns (keys are >= +0: the doubles' order is their bits'): steps of one
                # ulp (equal high words), of a low-word carry and of whole exponents, from +0,
                # the subnormals or 1.0
                steps = rng.choice(np.array([1, 2, 1 << 31, 1 << 33, 1 << 50], np.uint64), size=L)
                steps[0] = rng.integers(2)
                bits = np.uint64(rng.choice([0, 1 << 40, 0x3FF0000000000000])) + np.cumsum(steps, dtype=np.uint64)
                k = bits.view(np.float64)
                up = rng.choice(np.array([1, 1 << 33, 1 << 52], np.uint64), size=L)
                f = np.where(rng.integers(8, size=L) == 0, INF, (bits[L - 1] + up).view(np.float64))
                keep[b, s, g: g + gs] = rng.choice([0.0, 1.0, INF], size=gs)  # padding junk
                flip[b, s, g: g + gs] = rng.choice([0.0, 1.0, INF], size=gs)
                keep[b, s, g: g + L] = k
                flip[b, s, g: g + L] = f
    assert (np.diff(keep.reshape(nb, nsets, 64 // gs, gs)[..., :L], axis=-1) > 0).all()
    return keep, flip


def _spoil(rng, keep, flip, L, gs):
    """One group of each wave set loses the property by a single entry (a tie among the
    keeps, a flip equal to / below the largest keep, a descent)."""
    keep, flip = keep.copy(), flip.copy()
    for b in range(keep.shape[0]):
        for s in range(keep.shape[1]):
            g = gs * int(rng.integers(64 // gs))
            how = int(rng.integers(4))
            i = int(rng.integers(1, L))
            if how == 0:
                keep[b, s, g + i] = keep[b, s, g + i - 1]
            elif how == 1:
                flip[b, s, g + int(rng.integers(L))] = keep[b, s, g + L - 1]
            elif how == 2:
                flip[b, s, g + int(rng.integers(L))] = keep[b, s, g]
            else:
                keep[b, s, g + i - 1], keep[b, s, g + i] = keep[b, s, g + i], keep[b, s, g + i - 1]
    return keep, flip


@pytest.mark.parametrize("nsets", [1, 2])
@pytest.mark.parametrize("L", [8] + list(range(9, 17)))
def test_keep_all_identity(L, nsets, harness):
    """keep_all8 (L = 8) / keep_all16: a false "identity" silently drops a fork.
    Soundness: whenever the wave-uniform result is true, the reference selection of every
    group of the wave is the identity.  Completeness: strictly increasing keeps with every
    flip strictly above the largest keep give true.  Both outcomes must occur."""
    import sel_harness as S

    prim, gs = (S.KEEP8, 8) if L == 8 else (S.KEEP16, 16)
    rng = np.random.default_rng(77 * L + nsets)
    ik, iflip = _identity_waves(rng, L, gs, 192, nsets)
    sk, sf = _spoil(rng, ik[:96], iflip[:96], L, gs)
    if L == 8:
        rk = np.stack([rng.integers(3, size=(64, nsets, 64)).astype(np.float64), rng.choice(TINY, size=(64, nsets, 64))])
        rk = rk.reshape(128, nsets, 64)
        rf = rk + rng.integers(3, size=rk.shape)
    else:
        rk, rf = (a[:128] for a in _w16_case(harness, L, nsets)[:2])
    # sorted keeps with ties and flips >= the largest keep: the identity under a stable sort (2L <= 16) only
    tk = np.sort(rng.integers(4, size=(64, nsets, 64 // gs, gs)).astype(np.float64), axis=-1)
    tf = tk[..., L - 1: L] + rng.integers(3, size=tk.shape)
    keep = np.concatenate([ik, sk, rk, tk.reshape(64, nsets, 64)])
    flip = np.concatenate([iflip, sf, rf, tf.reshape(64, nsets, 64)])
    _, _, ident, canary = harness.run(prim, L, keep, flip)
    assert canary.all()
    assert (ident == ident[..., :1]).all(), "the identity result is not wave-uniform"
    got = ident[..., 0].astype(bool)  # [blocks, sets]
    wp, wu = harness.reference(L, gs, keep, flip)
    live = (np.arange(64) % gs) < L
    ref_identity = ((wp == np.arange(64) % gs) & (wu == 0))[..., live].all(-1)
    print(f"L={L} sets={nsets}: identity true {int(got.sum())} / false {int((~got).sum())}, "
          f"reference identities {int(ref_identity.sum())}")
    assert not (got & ~ref_identity).any(), f"false identity in waves {np.argwhere(got & ~ref_identity)[:8].tolist()}"
    assert got[:192].all(), f"identity missed in waves {np.argwhere(~got[:192])[:8].tolist()}"
    assert got.any() and (~got).any()
    if L > 8:
        assert not got[192:288].any()  # every spoiled wave is refused (each change breaks strictness)
    else:  # 2L = 16 sorts stably: ordered keeps with ties and flips >= the largest keep are the identity
        assert got[-64:].all(), f"identity missed in waves {np.argwhere(~got[-64:])[:8].tolist()}"


@pytest.mark.parametrize("nsets", [1, 2])
@pytest.mark.parametrize("L", range(1, 9))
def test_select_survivors_small_lists(L, nsets, harness):
    """select_survivors8 (L = 8) and the generic select_survivors (L = 1..8, lane groups of
    the power of two >= L): 2L <= 16, so std::sort is the stable insertion sort -- order by
    (key, candidate index) -- on tie-heavy, +inf and +0 keys."""
    import sel_harness as S

    rng = np.random.default_rng(31 * L + nsets)
    gs = harness.group_size(S.GENERIC, L)
    assert gs >= L and gs < 2 * L or L == 1
    nb = 256
    shape = (nb, nsets, 64)
    kinds = rng.integers(5, size=(nb, nsets, 64 // gs, 1)).repeat(gs, -1).reshape(shape)  # a class per group
    few = rng.integers(3, size=shape).astype(np.float64)
    keep = np.select([kinds == 0, kinds == 1, kinds == 2, kinds == 3],
                     [few, np.where(rng.integers(3, size=shape) == 0, INF, few), rng.choice(TINY, size=shape),
                      np.full(shape, 7.0)], rng.permutation(nb * nsets * 64).reshape(shape) + 0.5)
    pen = np.where(rng.integers(3, size=shape) == 0, 0.0, rng.integers(1, 3, size=shape))
    flip = np.where(kinds == 2, rng.choice(TINY, size=shape), keep + pen)
    if gs > L:  # padding lanes: junk the primitive must not read
        pad = (np.arange(64) % gs) >= L
        keep[..., pad] = rng.choice([0.0, INF], size=(nb, nsets, int(pad.sum())))
        flip[..., pad] = rng.choice([0.0, INF], size=(nb, nsets, int(pad.sum())))
    want = harness.reference(L, gs, keep, flip)
    prims = [(S.GENERIC, "select_survivors")] + ([(S.SEL8, "select_survivors8")] if L == 8 else [])
    for prim, name in prims:
        assert harness.group_size(prim, L) == gs
        parent, upper, _, canary = harness.run(prim, L, keep, flip)
        assert canary.all(), f"{name}: LDS canaries overwritten in blocks {np.flatnonzero(canary == 0)[:8]}"
        _assert_selection(parent, upper, want, L, gs, f"{name} L={L} sets={nsets}")
