"""The fast engine's rate-1 (R1) nodes, called directly on the device.

Every FastSCL-LUT / CA-FastSCL-LUT decode on the fast engine decides the bits of its R1
nodes in qpd_fast_special.hpp: r1_prep finds the first m = min(L - 1, temp) outputs of the
reference's std::sort argsort of |llr| (packed 16-bit min trees up to 16 elements; above,
partition_prefix_masked -- the introsort's partitions by ballot-driven masks, heap-sort
fallback at the depth limit -- then min trees over (rank, position, element)), r1_layers /
r1_multi fork on them and stop at the first identity layer.  A decode reaches only the rank
arrays its tables and frames happen to produce; the harness (tests/native/r1_harness.hip)
hands chosen symbols, rank tables, quanta and metrics to these functions themselves, one
array per lane, in an LDS layout between canary rows.

All comparisons are exact, against the harness library's host references (std::sort
itself).  Every case asserts the canaries and that no set's source rows changed.
"""
import functools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu

BLOCKS = 256       # one-wave blocks per argsort launch
NODE_BLOCKS = 128  # per node launch
N_CLASSES = 8
TEMPS = [1, 2, 7, 8, 9, 15, 16, 17, 18, 24, 30, 31, 32]  # (30: the size of one committed witness)
NODE_TEMPS = [4, 8, 16, 17, 32]


@pytest.fixture(scope="module")
def harness(native_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import r1_harness

    return r1_harness.load()  # rebuilt only when the harness or csrc/ changed


@pytest.fixture(scope="module")
def adversary(native_lib):
    import sel_harness

    return sel_harness.load().adversary


@functools.lru_cache(maxsize=None)
def _witnesses():
    with open(os.path.join(GOLDEN_DIR, "r1_heap_witnesses.json")) as fh:
        return json.load(fh)["witnesses"]


def _witness_base(temp, rng):
    """The committed witnesses of this size, or all of them cut / padded to it."""
    own = [np.array(w["ranks"]) for w in _witnesses() if w["n"] == temp]
    if own:
        return own
    out = []
    for w in _witnesses():
        r = np.array(w["ranks"])
        out.append(r[:temp] if temp <= r.size else np.concatenate([r, rng.integers(16, size=temp - r.size)]))
    return out


def _class_ranks(rng, cls, cnt, temp, adv):
    """cnt rank arrays (ranks < 16) of one key class: [cnt, temp]."""
    j = np.arange(temp)
    if cls == 0:  # all equal
        return np.repeat(rng.integers(16, size=(cnt, 1)), temp, axis=1)
    if cls == 1:  # 2-4 distinct ranks
        k = rng.integers(2, 5, size=(cnt, 1))
        vals = np.argsort(rng.random((cnt, 16)), axis=1)[:, :4]
        return np.take_along_axis(vals, rng.integers(0, 1 << 30, size=(cnt, temp)) % k, axis=1)
    if cls == 2:  # sorted
        return np.sort(rng.integers(16, size=(cnt, temp)), axis=1)
    if cls == 3:  # reversed
        return np.sort(rng.integers(16, size=(cnt, temp)), axis=1)[:, ::-1]
    if cls == 4:  # organ pipe, up or down
        pipe = np.minimum(15, np.where(j < temp // 2, j, temp - j))
        return np.where(rng.integers(2, size=(cnt, 1)) == 1, pipe, 15 - pipe)
    if cls == 5:  # a random permutation (<= 16 elements), else all 16 ranks at random
        if temp <= 16:
            return np.argsort(rng.random((cnt, temp)), axis=1)
        return rng.integers(16, size=(cnt, temp))
    if cls == 6:
        # McIlroy's adversary against std::sort of temp elements, or with one entry changed.  Above 16
        # elements this is a CAPPED variant (its keys 15..temp-1 fold into rank 15: ranks in the op
        # record are < 16); the adversary itself goes through the per-element table (_adversary_blocks)
        base = np.minimum(adv(temp), 15).astype(np.int64) if temp >= 2 else np.zeros(1, np.int64)
        out = np.repeat(base[None, :], cnt, axis=0)
        ch = rng.integers(2, size=cnt) == 1
        out[ch, rng.integers(temp, size=cnt)[ch]] = rng.integers(16, size=cnt)[ch]
        return out
    # the committed depth-limit witnesses and their single-entry mutations
    base = np.stack(_witness_base(temp, rng))
    out = base[rng.integers(len(base), size=cnt)].copy()
    ch = rng.integers(3, size=cnt) == 0
    out[ch, rng.integers(temp, size=cnt)[ch]] = rng.integers(16, size=cnt)[ch]
    return out


_RANKS = {}


def _ranks(temp, adv):
    """[BLOCKS, 2, 64, temp] rank arrays, every class in every lane position; shared by the cases
    of this temp (one set: the first of the two)."""
    if temp not in _RANKS:
        rng = np.random.default_rng(7000 + temp)
        b, s, lane = np.meshgrid(np.arange(BLOCKS), np.arange(2), np.arange(64), indexing="ij")
        cls = (b + 3 * s + lane) % N_CLASSES
        R = np.empty((BLOCKS, 2, 64, temp), np.int64)
        for c in range(N_CLASSES):
            mask = cls == c
            R[mask] = _class_ranks(rng, c, int(mask.sum()), temp, adv)
        _RANKS[temp] = R
    return _RANKS[temp]


def _tables(src, ranks, v=16):
    """Rank tables and symbols that give every lane its rank array.  RK / VUNI: one rank row per
    block, a permutation of the 16 ranks over the symbols with random signs; TAB: a row per
    element, each its own permutation, the ranks spread strictly monotonically below 2047."""
    import r1_harness as R

    nb, ns, _, temp = ranks.shape
    rng = np.random.default_rng(11 * temp + src)
    sign = rng.integers(2, size=(nb, temp if src == R.SRC_TAB else 1, v))
    perm = np.argsort(rng.random(sign.shape), axis=2)  # perm[b, j, symbol] = rank
    if src != R.SRC_TAB:
        perm, sign = np.repeat(perm, temp, axis=1), np.repeat(sign, temp, axis=1)
    inv = np.argsort(perm, axis=2)                      # inv[b, j, rank] = symbol
    sym = inv[np.arange(nb)[:, None, None, None], np.arange(temp)[None, None, None, :], ranks]
    wide = perm
    if src == R.SRC_TAB:
        spread = np.sort(np.argsort(rng.random((nb, 2047)), axis=1)[:, :16], axis=1)  # [b, rank] -> wide rank
        wide = spread[np.arange(nb)[:, None, None], perm]
    return ((wide << 1) | sign).astype(np.uint16), sym.astype(np.uint8)


N_ADV = 16  # blocks of the per-element-table cases that hold the uncapped adversary (temp > 16)


def _adversary_blocks(temp, ns, adv):
    """McIlroy's adversary against std::sort of temp > 16 elements, uncapped (keys up to temp - 1),
    through the per-element rank table: row j of a block offers the adversary's key of element j
    and 15 other keys of the sequence, on symbols permuted per row.  Every fourth lane holds the
    adversary itself, the others one to three entries moved to another key of their row."""
    rng = np.random.default_rng(900 + temp)
    val = adv(temp).astype(np.int64)
    keys = np.empty((N_ADV, temp, 16), np.int64)
    for b in range(N_ADV):
        for j in range(temp):
            others = rng.permutation(np.setdiff1d(np.arange(temp), [val[j]]))[:15]
            keys[b, j] = rng.permutation(np.concatenate([[val[j]], others]))
    own = np.argmax(keys == val[None, :, None], axis=2)  # [b, j]: the symbol of the adversary's key
    sym = np.repeat(own[:, None, None, :], ns, axis=1).repeat(64, axis=2)
    lane = np.arange(64)
    for k in range(3):
        ch = (lane % 4 != 0)[None, None, :] & (rng.integers(k + 1, size=(N_ADV, ns, 64)) == 0)
        pos = rng.integers(temp, size=(N_ADV, ns, 64))
        bi, si, li = np.nonzero(ch)
        sym[bi, si, li, pos[bi, si, li]] = rng.integers(16, size=bi.size)
    sign = rng.integers(2, size=keys.shape)
    return ((keys << 1) | sign).astype(np.uint16), sym.astype(np.uint8)


def _inst_for(L, src):
    import r1_harness as R

    if L > 8:
        return [R.GEN15]
    return [R.GEN7, R.RK7] if src == R.SRC_RK else [R.GEN7]


def _min_witness_m(temp):
    ms = [min(w["m"]) for w in _witnesses() if w["n"] == temp and w["m"]]
    return min(ms) if ms else None


@pytest.mark.parametrize("ns", [1, 2])
@pytest.mark.parametrize("src", [0, 1, 2], ids=["rk", "vuni", "tab"])
@pytest.mark.parametrize("L", [2, 4, 7, 8, 9, 12, 13, 16])  # m = 1, 3, 6, 7, 8, 11, 12, 15 (or temp)
@pytest.mark.parametrize("temp", TEMPS)
def test_r1_argsort(harness, adversary, temp, L, src, ns):
    """r1_prep's first m outputs, their symbols and the hard-decision word against std::sort on
    the lane's rank array, for every instantiation that serves (L, rank source)."""
    import r1_harness as R

    ranks = _ranks(temp, adversary)[:, :ns]
    m = min(L - 1, temp)
    table, sym = _tables(src, ranks)
    if src == R.SRC_TAB and temp > 16:
        table[-N_ADV:], sym[-N_ADV:] = _adversary_blocks(temp, ns, adversary)
    # the lanes' rank arrays as the kernel sees them; its hard decisions are the symbols' sign bits
    entry = table[np.arange(BLOCKS)[:, None, None, None], np.arange(temp)[None, None, None, :], sym]
    if src != R.SRC_TAB:
        assert np.array_equal(entry >> 1, ranks)
    ranks = (entry >> 1).astype(np.int64)
    if temp > 16:
        # conditions on the inputs, from the host predicate: lanes of one wave differ in their
        # partition counts; where a committed witness of this size falls back at this m, some lane
        # takes the natural heap-sort fallback, beside lanes of its wave that partition to a natural end
        fell, parts = harness.heap(ranks, m)
        waves_mixed = int((fell.any(axis=2) & ~fell.all(axis=2)).sum())
        print(f"temp={temp} L={L} m={m}: natural fallbacks {int(fell.sum())} lanes, mixed waves {waves_mixed}, "
              f"partition counts {int(parts.min())}..{int(parts.max())}")
        if temp >= 24:  # (17, 18: one partition leaves no range above the threshold in play)
            assert (parts.max(axis=2) > parts.min(axis=2)).any()
        wm = _min_witness_m(temp)
        if wm is not None and m >= wm:
            assert fell.any() and waves_mixed > 0
    want_ord, want_sym, want_hw = harness.argsort_ref(L, 16, table, sym)
    hw = ((entry & 1).astype(np.uint64) << np.arange(temp, dtype=np.uint64)).sum(axis=3).astype(np.uint32)
    assert np.array_equal(want_hw, hw)
    assert (want_ord[..., m:] == -1).all() and (want_ord[..., :m] >= 0).all()
    for inst in _inst_for(L, src):
        got_ord, got_sym, got_hw, ok = harness.argsort(inst, src, L, 16, table, sym)
        assert (ok == 3).all(), f"canaries / source rows: blocks {np.flatnonzero(ok != 3)[:8]} flags {ok[ok != 3][:8]}"
        bad = np.argwhere((got_ord != want_ord).any(axis=3))
        assert bad.size == 0, (f"inst {inst}: {len(bad)} lanes differ, first (block, set, lane) {bad[0]}: ranks "
                               f"{ranks[tuple(bad[0])]} got {got_ord[tuple(bad[0])]} want {want_ord[tuple(bad[0])]}")
        assert np.array_equal(got_sym, want_sym)
        assert np.array_equal(got_hw, hw) and not (got_hw >> np.uint32(temp) if temp < 32 else got_hw * 0).any()


def test_r1_heap_fallback_is_exercised(harness, adversary):
    """The counts the argsort cases rest on: with the committed witnesses among the lanes, the
    natural heap-sort fallback of partition_prefix_masked is taken at sizes 30, 31 and 32 (the
    production node size at N = 1024, the one size with depth limit 10), in waves whose other
    lanes partition to a natural end."""
    total = 0
    for temp, L in ((31, 8), (31, 9), (31, 16), (30, 9), (30, 16), (32, 12), (32, 16)):
        fell, _ = harness.heap(_ranks(temp, adversary), min(L - 1, temp))
        mixed = int((fell.any(axis=2) & ~fell.all(axis=2)).sum())
        print(f"temp={temp} L={L}: {int(fell.sum())} fallback lanes, {mixed} mixed waves")
        assert fell.sum() > 0 and mixed > 0
        total += int(fell.sum())
    assert total > 0


# --------------------------------------------------------------------------------------------
# whole nodes
# --------------------------------------------------------------------------------------------
def _node_case(L, temp, ns, gs):
    """Quanta rows, metrics and symbols of NODE_BLOCKS waves.  Blocks b % 4 == 0 are identity
    blocks (every group of every set is built so that layer 0 is the identity: the wave takes the
    early-out); in the others every fourth group is, beside groups of the other metric classes."""
    rng = np.random.default_rng(100000 + 1000 * L + 10 * temp + ns)
    nb, v, ng = NODE_BLOCKS, 16, 64 // gs
    nmag = rng.integers(2, 5, size=nb)
    mags = rng.choice([0.25, 0.5, 0.75, 1.0, 1.5, 0.1, 0.3, 2.7], size=(nb, 4))
    quanta = np.take_along_axis(mags, rng.integers(0, 1 << 30, size=(nb, v)) % nmag[:, None], axis=1)
    zero = (np.arange(nb) % 4 == 1)[:, None] & (rng.integers(3, size=(nb, v)) == 0)  # rows with exact 0.0
    quanta = np.where(zero, 0.0, quanta) * np.where(rng.integers(2, size=(nb, v)) == 1, -1.0, 1.0)
    mmin = np.abs(quanta).min(axis=1)  # > 0 except in the rows with zeros
    sym = rng.integers(v, size=(nb, ns, 64, temp))
    same = rng.integers(8, size=(nb, ns, 64)) == 0  # some paths: one symbol throughout
    sym[same] = sym[same][:, :1]
    pm = np.full((nb, ns, ng, gs), np.inf)
    ident = np.zeros((nb, ns, ng), bool)
    for b in range(nb):
        for s in range(ns):
            for g in range(ng):
                cls = 0 if (b % 4 == 0 or (g % 4 == 3 and mmin[b] > 0)) else 1 + int(rng.integers(4))
                if cls == 0:
                    # ascending metrics whose spread the smallest magnitude exceeds (L <= 8: ties
                    # allowed, in the metrics and between the first flip and the last keep)
                    ident[b, s, g] = True
                    base = float(rng.integers(8)) * 0.5
                    if L <= 8 and rng.integers(2):
                        steps = np.sort(rng.integers(0, 3, size=L)) / 2.0
                        steps[0] = 0.0
                        k = base + steps * mmin[b]
                        if L > 1 and rng.integers(2):
                            k[L - 1] = k[0] + mmin[b]
                    else:
                        k = base + np.arange(L) * (mmin[b] / (L + 1))
                elif cls == 1:  # small multiples: ties among keeps and flips
                    k = rng.integers(4, size=L) * 0.25
                elif cls == 2:  # all equal
                    k = np.full(L, float(rng.integers(3)))
                elif cls == 3:  # dead paths
                    k = np.where(np.arange(L) < 1 + rng.integers(L), rng.integers(3, size=L) * 0.5, np.inf)
                else:  # anything
                    k = rng.random(L) * 3
                pm[b, s, g, :L] = k
    return quanta, pm.reshape(nb, ns, 64), sym.astype(np.uint8), ident


def _node_modes(L):
    import r1_harness as R

    if L < 8:
        return [(R.SMALL0, s) for s in (R.SRC_RK, R.SRC_VUNI, R.SRC_TAB)]
    if L == 8:  # (r1_small<0> too: the generic selection on a full group of 8)
        return ([(R.MULTI, R.SRC_RK), (R.SMALL0, R.SRC_RK)] + [(R.MULTI_GEN, s) for s in (R.SRC_RK, R.SRC_VUNI, R.SRC_TAB)]
                + [(R.SMALL8, s) for s in (R.SRC_RK, R.SRC_VUNI, R.SRC_TAB)])
    return [(R.SMALL16, s) for s in (R.SRC_RK, R.SRC_VUNI, R.SRC_TAB)]


@pytest.mark.parametrize("ns", [1, 2])
@pytest.mark.parametrize("temp", NODE_TEMPS)
@pytest.mark.parametrize("L", [1, 2, 3, 4, 6, 8, 9, 13, 16])  # (6: groups of 8 with padding lanes)
def test_r1_node(harness, L, temp, ns):
    """A whole R1 node through r1_small<LM> / r1_multi: node word, metrics (bit patterns) and
    lineage against the reference, on every rank source; the identity early-out on groups and
    waves built for it."""
    gs = harness.group_size(L)
    m = min(L - 1, temp)
    quanta, pm, sym, ident = _node_case(L, temp, ns, gs)
    w_word, w_pm, w_lin, w_id = harness.node_ref(L, quanta, pm, sym)
    live = np.tile(np.arange(gs) < L, 64 // gs)
    idm = w_id.reshape(NODE_BLOCKS, ns, 64 // gs, gs)[..., 0]
    full = np.uint32((1 << m) - 1)
    if m > 0:
        # from the reference: a group built with an identity first layer has every later layer the
        # identity too (what the early-out rests on); both kinds of first layer occur
        assert ((idm[ident] & 1) == 1).all()
        assert (idm[ident] == full).all()
        if L <= 8:
            # ... and whatever the class (stable selection): the non-identity layers are the first ones
            non = ~idm & full
            assert ((non & (non + np.uint32(1))) == 0).all(), "an identity layer is followed by a non-identity one"
        n_id, n_non = int((idm & 1).sum()), int(((idm & 1) == 0).sum())
        waves_id = int(((idm & 1) == 1).all(axis=(1, 2)).sum())
        print(f"L={L} temp={temp} ns={ns}: first layer identity in {n_id} groups ({waves_id} whole waves), not in {n_non}")
        assert n_id > 0 and n_non > 0 and waves_id > 0
    tmask = np.uint32((1 << temp) - 1 if temp < 32 else 0xFFFFFFFF)
    for mode, src in _node_modes(L):
        word, pmo, lin, ok = harness.node(mode, src, L, quanta, pm, sym)
        assert (ok == 3).all(), f"mode {mode} src {src}: canaries / source rows, blocks {np.flatnonzero(ok != 3)[:8]}"
        bad = np.argwhere(((word & tmask) != w_word)[..., live])
        assert bad.size == 0, f"mode {mode} src {src}: {len(bad)} node words differ, first {bad[0]}"
        assert np.array_equal(pmo[..., live].view(np.uint64), w_pm[..., live].view(np.uint64)), f"mode {mode} src {src}: metrics"
        assert np.array_equal(lin[..., live], w_lin[..., live]), f"mode {mode} src {src}: lineage"


# --------------------------------------------------------------------------------------------
# the references themselves, and the entry points' refusals
# --------------------------------------------------------------------------------------------
def test_r1_references_match_numpy(harness):
    """On tie-free inputs every correct sort agrees: the host references equal a numpy
    implementation built on np.argsort(kind="stable")."""
    rng = np.random.default_rng(5)
    for temp, L in ((5, 4), (16, 8), (17, 16), (32, 12)):
        nb, m = 4, min(L - 1, temp)
        # all-distinct ranks through the per-element table
        wide = np.argsort(rng.random((nb, temp * 16)), axis=1).reshape(nb, temp, 16)
        table = ((wide << 1) | rng.integers(2, size=wide.shape)).astype(np.uint16)
        sym = rng.integers(16, size=(nb, 1, 64, temp)).astype(np.uint8)
        o, sy, hw = harness.argsort_ref(L, 16, table, sym)
        entry = table[np.arange(nb)[:, None, None, None], np.arange(temp)[None, None, None, :], sym]
        want = np.argsort(entry >> 1, axis=3, kind="stable")[..., :m]
        assert np.array_equal(o[..., :m], want)
        assert np.array_equal(sy[..., :m], np.take_along_axis(sym, want, axis=3))
        assert np.array_equal(hw, ((entry & 1).astype(np.uint64) << np.arange(temp, dtype=np.uint64)).sum(axis=3))
    for temp, L in ((4, 3), (8, 8), (16, 16), (16, 9)):
        nb, gs, m = 3, harness.group_size(L), min(L - 1, temp)
        quanta = (rng.random((nb, 16)) + 0.01) * np.where(rng.integers(2, size=(nb, 16)) == 1, -1.0, 1.0)
        sym = np.argsort(rng.random((nb, 1, 64, 16)), axis=3)[..., :temp].astype(np.uint8)  # distinct symbols per path
        pm = rng.random((nb, 1, 64)) * 2
        word, pmo, lin, _ = harness.node_ref(L, quanta, pm, sym)
        for b in range(nb):
            for g in range(0, 64, gs):
                llr = quanta[b][sym[b, 0, g:g + L]]  # [L, temp]
                mag, hard = np.abs(llr), (llr < 0).astype(np.int64)
                order = np.argsort(mag, axis=1, kind="stable")
                cur, origin, flips = pm[b, 0, g:g + L].copy(), np.arange(L), np.zeros((L, temp), np.int64)
                for q in range(m):
                    pos = order[origin, q]
                    key = np.concatenate([cur, cur + mag[origin, pos]])
                    assert np.unique(key).size == 2 * L
                    idx = np.argsort(key, kind="stable")[:L]
                    par = idx % L
                    nf = flips[par].copy()
                    nf[idx >= L, pos[idx >= L]] ^= 1  # (H2: the slot's own pre-selection position)
                    cur, origin, flips = key[idx], origin[par], nf
                bits = hard[origin] ^ flips
                assert np.array_equal(word[b, 0, g:g + L], (bits << np.arange(temp)).sum(axis=1))
                assert np.array_equal(pmo[b, 0, g:g + L], cur) and np.array_equal(lin[b, 0, g:g + L], origin)


def test_r1_entry_points_refuse(harness):
    """Nothing the kernels cannot run is launched: -1 before any launch."""
    import r1_harness as R

    def args(temp=8, v=16, ns=1, nb=2, rank_max=16):
        rng = np.random.default_rng(1)
        row = ((rng.integers(rank_max, size=(nb, 1, v)) << 1) | 1).astype(np.uint16)
        return np.repeat(row, temp, axis=1), rng.integers(v, size=(nb, ns, 64, temp)).astype(np.uint8)

    t, s = args()
    assert harness.argsort_raw(R.GEN7, R.SRC_RK, 8, 8, 16, 1, 2, t, s) == 0
    for temp in (0, 33):  # temp outside 1..32
        tt, ss = args(temp=max(temp, 1))
        assert harness.argsort_raw(R.GEN7, R.SRC_RK, 8, temp, 16, 1, 2, tt, ss) == -1
    for L in (0, 17, -3):  # L outside 1..16
        assert harness.argsort_raw(R.GEN15, R.SRC_RK, L, 8, 16, 1, 2, t, s) == -1
    for ns in (0, 3):  # set counts other than 1, 2
        tt, ss = args(ns=max(ns, 1))
        assert harness.argsort_raw(R.GEN7, R.SRC_RK, 8, 8, 16, ns, 2, tt, ss) == -1
    assert harness.argsort_raw(R.GEN7, R.SRC_RK, 9, 8, 16, 1, 2, t, s) == -1   # m = 8 above MAXM = 7
    assert harness.argsort_raw(R.RK7, R.SRC_RK, 16, 16, 16, 1, 2, *args(temp=16)) == -1
    assert harness.argsort_raw(R.GEN15, R.SRC_RK, 16, 16, 16, 1, 2, *args(temp=16)) == 0
    assert harness.argsort_raw(R.RK7, R.SRC_VUNI, 8, 8, 16, 1, 2, t, s) == -1  # GEN = false: op-record ranks only
    tt, ss = args(rank_max=40)
    tt[0, :, 3] = (17 << 1)
    assert harness.argsort_raw(R.GEN7, R.SRC_RK, 8, 8, 16, 1, 2, tt, ss) == -1   # ranks >= 16 with MF_R1_RK
    assert harness.argsort_raw(R.GEN7, R.SRC_TAB, 8, 8, 16, 1, 2, tt, ss) == 0   # ... fine in the rank table
    tt, ss = args()
    tt[1, 3, 2] ^= 2
    assert harness.argsort_raw(R.GEN7, R.SRC_VUNI, 8, 8, 16, 1, 2, tt, ss) == -1  # one rank row: rows differ
    tt, ss = args(v=8)
    ss[1, 0, 5, 2] = 8
    assert harness.argsort_raw(R.GEN7, R.SRC_RK, 8, 8, 8, 1, 2, tt, ss) == -1    # symbols >= v
    assert harness.argsort_raw(7, R.SRC_RK, 8, 8, 16, 1, 2, t, s) == -1 and harness.argsort_raw(R.GEN7, 5, 8, 8, 16, 1, 2, t, s) == -1
    assert harness.argsort_raw(R.GEN7, R.SRC_RK, 8, 8, 16, 1, 0, t, s) == -1

    q = np.tile(np.linspace(-1.0, 1.0, 16), (2, 1))
    pm = np.zeros((2, 1, 64))
    assert harness.node_raw(R.SMALL8, R.SRC_RK, 8, 8, 16, 1, 2, q, pm, s) == 0
    assert harness.node_raw(R.SMALL8, R.SRC_RK, 8, 33, 16, 1, 2, q, pm, s) == -1
    assert harness.node_raw(R.SMALL8, R.SRC_RK, 8, 0, 16, 1, 2, q, pm, s) == -1
    assert harness.node_raw(R.SMALL0, R.SRC_RK, 9, 8, 16, 1, 2, q, pm, s) == -1    # the generic selection: L <= 8
    assert harness.node_raw(R.SMALL8, R.SRC_RK, 4, 8, 16, 1, 2, q, pm, s) == -1    # groups of 8: L = 8
    assert harness.node_raw(R.MULTI, R.SRC_RK, 7, 8, 16, 1, 2, q, pm, s) == -1
    assert harness.node_raw(R.MULTI, R.SRC_VUNI, 8, 8, 16, 1, 2, q, pm, s) == -1   # GEN = false: op-record ranks only
    assert harness.node_raw(R.SMALL16, R.SRC_RK, 8, 8, 16, 1, 2, q, pm, s) == -1   # groups of 16: L = 9..16
    assert harness.node_raw(R.SMALL16, R.SRC_RK, 17, 8, 16, 1, 2, q, pm, s) == -1
    assert harness.node_raw(R.SMALL8, R.SRC_RK, 8, 8, 16, 3, 2, q, pm, s) == -1
    assert harness.node_raw(9, R.SRC_RK, 8, 8, 16, 1, 2, q, pm, s) == -1
    bad = pm.copy()
    bad[1, 0, 9] = np.nan
    assert harness.node_raw(R.SMALL8, R.SRC_RK, 8, 8, 16, 1, 2, q, bad, s) == -1   # NaN / negative metrics
    bad[1, 0, 9] = -1.0
    assert harness.node_raw(R.SMALL8, R.SRC_RK, 8, 8, 16, 1, 2, q, bad, s) == -1
    s2 = s.copy()
    s2[0, 0, 0, 0] = 16
    assert harness.node_raw(R.SMALL8, R.SRC_RK, 8, 8, 16, 1, 2, q, pm, s2) == -1   # symbols >= v
