"""The Monte-Carlo generator's own arithmetic on the device (csrc/qpd_mc.hip: philox4x32_10,
mc_one_m, mc_log, mc_sincos and the Box-Muller step built from them), through the harness
tests/native/mc_math_harness.hip, against mpmath at 200 bits on the exact input doubles.

The generator's tests reach these functions through about 10^5 LLRs each; a 10^8-frame point
draws 5 * 10^10 pairs and does meet u1 = 2^-52 (radius 8.49), u1 = 1 (log 0), every binade
boundary of u1, a log mantissa next to sqrt(1/2) and angles next to the multiples of pi/2.
Those inputs are built here, with 50 000 random draws, in one launch.

Bounds -- the project's own claims, not figures taken from the code under test:
  mc_log        1 ulp of the reference      (the comment in qpd_mc.hip: fdlibm, < 1 ulp)
  sin, cos      2^-52 absolute              (1 ulp at 1: they only ever multiply the radius)
  nz            2e-14 absolute              (the |d nz| the 2e-13 / sigma LLR bound of
                                             test_gpu_mc_llr.py::test_llrs_match_restatement is 5x of)
Measured on the MI355X (printed by the test): see DESIGN.md row (f) F2."""
import math

import numpy as np
import pytest

import mc_ref

pytestmark = pytest.mark.gpu

TWO52 = 1 << 52


@pytest.fixture(scope="module")
def harness(native_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import mc_math_harness

    return mc_math_harness.load()


def words_of(m, rng):
    """Two Philox words whose 52 mantissa bits (a >> 12) : b are m; the 12 bits mc_one_m drops are random."""
    m = np.asarray(m, dtype=np.uint64)
    a = ((m >> np.uint64(32)) << np.uint64(12)) | rng.integers(0, 1 << 12, size=m.size, dtype=np.uint64)
    return a.astype(np.uint32), (m & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def edge_mantissas():
    """(m1, m2): the 52-bit mantissas of the edge inputs.  u1 = (2^52 - m1) / 2^52, u2 = m2 / 2^52."""
    j = {1, TWO52}  # u1 = j / 2^52: 2^-52 and 1
    for k in range(52):
        j.update(2 ** k + d for d in range(-2, 3))  # every binade boundary of u1
    for k in range(3, 52):  # the log's mantissa (frexp, doubled below sqrt(1/2)) within 4 steps of sqrt(1/2)
        j.update(math.isqrt(1 << (2 * k + 1)) + d for d in range(-4, 5))
    m1 = sorted(TWO52 - x for x in j if 1 <= x <= TWO52)
    m2 = {0, TWO52 - 1}
    for e in range(9):  # the angle next to the multiples of pi / 4 (pi / 2: where sin / cos vanish)
        m2.update(e * (1 << 49) + d for d in range(-2, 3))
    m2 = sorted(x for x in m2 if 0 <= x < TWO52)
    return np.array(m1, dtype=np.uint64), np.array(m2, dtype=np.uint64)


def inputs():
    rng = np.random.default_rng(52)
    m1, m2 = edge_mantissas()
    # every edge u1 with every edge u2 (u1 = 2^-52, the largest radius, with every edge angle)
    g1, g2 = np.repeat(m1, m2.size), np.tile(m2, m1.size)
    a, b = words_of(g1, rng)
    c, d = words_of(g2, rng)
    r = rng.integers(0, 1 << 32, size=(4, 50000), dtype=np.uint64).astype(np.uint32)
    # the edges of one argument with random values of the other
    n = 4 * (m1.size + m2.size)
    ea, eb = words_of(np.concatenate([np.tile(m1, 4), rng.integers(0, TWO52, size=4 * m2.size, dtype=np.uint64)]), rng)
    ec, ed = words_of(np.concatenate([rng.integers(0, TWO52, size=4 * m1.size, dtype=np.uint64), np.tile(m2, 4)]), rng)
    assert ea.size == n
    return tuple(np.concatenate(x) for x in ((a, ea, r[0]), (b, eb, r[1]), (c, ec, r[2]), (d, ed, r[3])))


@pytest.fixture(scope="module")
def run(harness):
    a, b, c, d = inputs()
    assert 8e4 <= a.size <= 1.2e5
    return (a, b, c, d), harness.noise(a, b, c, d)


def test_uniforms_are_the_restatements(run):
    (a, b, c, d), out = run
    u1 = 2.0 - mc_ref.one_m(a, b)
    u2 = mc_ref.one_m(c, d) - 1.0
    assert np.array_equal(out["u1"], u1) and np.array_equal(out["u2"], u2)
    assert u1.min() == 2.0 ** -52 and u1.max() == 1.0 and u2.min() == 0.0 and u2.max() == 1.0 - 2.0 ** -52


def test_everything_is_finite_and_log_of_one_is_zero(run):
    _, out = run
    for name, x in out.items():
        assert np.isfinite(x).all(), name
    one = out["u1"] == 1.0
    assert one.sum() >= 40  # with every edge angle
    assert (out["log"][one] == 0).all() and (out["nz0"][one] == 0).all() and (out["nz1"][one] == 0).all()
    assert (out["log"] <= 0).all()


def test_against_mpmath(run):
    import mpmath

    _, out = run
    mp = mpmath.mp.clone()
    mp.prec = 200
    u1, ang = out["u1"], np.float64(6.283185307179586) * out["u2"]
    # one reference per distinct input double
    logs = {x: mp.log(mp.mpf(x)) for x in np.unique(u1).tolist()}
    trig = {x: mp.cos_sin(mp.mpf(x)) for x in np.unique(ang).tolist()}
    rads = {x: mp.sqrt(-2 * v) for x, v in logs.items()}
    worst = {"log": (0.0, None), "sin": (0.0, None), "cos": (0.0, None), "nz": (0.0, None)}

    def note(name, err, i):
        if err > worst[name][0]:
            worst[name] = (err, i)

    dev = {k: v.tolist() for k, v in out.items()}
    u1l, angl = u1.tolist(), ang.tolist()
    for i in range(len(u1l)):
        lg, (cs, sn), rad = logs[u1l[i]], trig[angl[i]], rads[u1l[i]]
        if lg != 0:
            ulp = mp.ldexp(1, int(mp.floor(mp.log(abs(lg), 2))) - 52)  # of a double next to the reference
            note("log", float(abs(mp.mpf(dev["log"][i]) - lg) / ulp), i)
        note("sin", float(abs(mp.mpf(dev["sin"][i]) - sn)), i)
        note("cos", float(abs(mp.mpf(dev["cos"][i]) - cs)), i)
        note("nz", float(max(abs(mp.mpf(dev["nz0"][i]) - rad * cs), abs(mp.mpf(dev["nz1"][i]) - rad * sn))), i)
    for name, (err, i) in worst.items():
        at = "" if i is None else f" at u1 = {u1l[i]!r} ({u1l[i].hex()}), angle = {angl[i]!r} ({angl[i].hex()})"
        print(f"mc math: max {name} error = {err:.4g}{' ulp' if name == 'log' else ''}{at}")
    assert worst["log"][0] <= 1.0, worst["log"]
    assert worst["sin"][0] <= 2.0 ** -52, worst["sin"]
    assert worst["cos"][0] <= 2.0 ** -52, worst["cos"]
    assert worst["nz"][0] <= 2e-14, worst["nz"]


def test_philox_known_answers_and_restatement(harness):
    """The two Random123 known-answer vectors (tests/test_montecarlo.py checks the restatement against them)
    and 1000 random (counter, key) inputs against the restatement, exactly; several counters under one key."""
    m = 0xFFFFFFFF
    got = harness.philox(np.array([[0, 0], [m, m]]), np.array([[[0, 0, 0, 0]], [[m, m, m, m]]]))
    assert [hex(x) for x in got[0, 0]] == [hex(x) for x in (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)]
    assert [hex(x) for x in got[1, 0]] == [hex(x) for x in (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)]
    rng = np.random.default_rng(10)
    for nk, nc in ((1000, 1), (3, 130)):
        keys = rng.integers(0, 1 << 32, size=(nk, 2), dtype=np.uint64).astype(np.uint32)
        ctr = rng.integers(0, 1 << 32, size=(nk, nc, 4), dtype=np.uint64).astype(np.uint32)
        got = harness.philox(keys, ctr)
        for k in range(nk):
            want = mc_ref.philox(ctr[k, :, 0], ctr[k, :, 1], ctr[k, :, 2], ctr[k, :, 3], int(keys[k, 0]), int(keys[k, 1]))
            assert np.array_equal(got[k], np.stack(want, axis=1).astype(np.uint32)), (nk, k)
