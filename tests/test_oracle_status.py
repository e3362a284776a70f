"""The oracle's decode status (oracle.decode_lut_status / decode_float_status:
every path's final metric, the output path, the CRC verdict, the CRC mask) pinned
on the CPU before tests/test_gpu_status_sweep.py compares the kernels with it:

* its bits are those of decode_lut / decode_lut_ca / decode_float on the grids of
  the GPU parity tests (one epilogue serves both families of calls);
* SCL-LUT and CA-SCL-LUT against tests/status_ref.py, the independent restatement
  of the reference's walk, L <= 8: bits, winner, verdict, and every metric as the
  same double; masks of 0, 1, 16 and crc_n bits, CRC11, K - A < crc_n;
* float CA-SCL against the reference's own recorded (bits, PM, isPass) of
  tests/golden/bd/bd_*.npz, L up to 32;
* every case of the sweep against the host engine (tests/native/status_harness.cpp).

For FastSCL-LUT, CA-FastSCL-LUT, the float kinds SCL and FastSCL and every L > 8
LUT case the final metric has no recorded reference value.  There it rests on two
independently written implementations agreeing bit for bit -- the oracle walks the
tree as the reference does, with the reference's own std::sort; the host engine
runs the compiled schedule with its replayed sort -- and on the decoded bits being
reference-exact on tie-heavy tables, where the order of the metrics decides the bits.
SCL-Uniform and SCL-Lloyd are not the host engine's: their metric rests on the
oracle alone (the SCL walk after a re-quantizer of the channel values, which the
float tests hold reference-exact in its bits), with no second implementation.

Also here, because they need no GPU: the conditions that keep the sweep's
comparisons informative (status_cases.check_informative), and the kernel
instantiation each sweep case reaches, planned on the CPU (status_cases.EXPECT).
"""
import glob
import os

import numpy as np
import pytest

import status_cases as S
import status_ref
import test_plan as TP
from conftest import GOLDEN_DIR, load_golden
from test_status_host import bd_groups, build_status_harness, host_status

BD_FILES = sorted(glob.glob(os.path.join(GOLDEN_DIR, "bd", "bd_*.npz")))
REF_KEYS = list(dict.fromkeys(c.ref_key() for c in S.CASES))
QPD_E_UNSUPPORTED = -2


@pytest.fixture(scope="module")
def harness():
    return build_status_harness()


@pytest.fixture(scope="module")
def plan_harness():
    return TP.load_harness()


def same(got, want):
    """bits, pml, winner and passed equal; the doubles as doubles."""
    return all(a.shape == b.shape and (a == b).all() for a, b in zip(got, want))


# -- bits unchanged -----------------------------------------------------------------------------------------

def test_bits_unchanged_lut(oracle_mod):
    from test_gpu_parity import CASES

    for N, K, L, tables in CASES:
        if L < 2:
            continue
        c = S.Case("SCL-LUT", N, K, L, tables, B=24 if N >= 1024 else 64)
        fm, nt, _ = S.code_of(c)
        for kind in ("SCL-LUT", "FastSCL-LUT"):
            if S.special_root(c._replace(kind=kind)):
                with pytest.raises(RuntimeError):
                    oracle_mod.decode_lut_status(kind, S.tables_of(c), K, L, fm, S.inputs_of(c), node_type=nt)
                continue
            want = oracle_mod.decode_lut(kind, S.tables_of(c), K, L, fm, S.inputs_of(c), node_type=nt)
            got = oracle_mod.decode_lut_status(kind, S.tables_of(c), K, L, fm, S.inputs_of(c), node_type=nt)
            assert (got[0] == want).all(), (kind, N, K, L, tables)
            assert not got[3].any() and (got[2] == got[1].argmin(1)).all()  # no CRC: the first minimum


def test_bits_unchanged_lut_ca(oracle_mod):
    for N, A, crc_n, L, tables, K in S.CA_ROWS:
        for kind in ("CA-SCL-LUT", "CA-FastSCL-LUT"):
            if S.special_root(S.Case(kind, N, K, L)):
                continue
            c = S._ca(kind, N, A, crc_n, L, tables, K=K)
            fm, nt, _ = S.code_of(c)
            kw = dict(node_type=nt, crc_n=crc_n, crc_loc=c.crc_loc)
            want = oracle_mod.decode_lut_ca(kind, S.tables_of(c), c.K, A, L, fm, S.inputs_of(c), **kw)
            assert (S.reference(c)[1][0][0] == want).all(), c.id


def test_bits_unchanged_float(oracle_mod):
    from test_float_oracle import float_inputs, quant_for
    from test_gpu_float import CASES

    for N, K, L in CASES:
        if L < 2:
            continue
        c = S.Case("SCL", N, K, L)
        fm, nt, _ = S.code_of(c)
        for style in ("awgn", "ties"):
            llr = float_inputs(N, 24 if N >= 1024 else 64, seed=N + L, style=style)
            for kind in S.FLOAT_KINDS:
                if (kind == "CA-SCL" and K < 16) or S.special_root(c._replace(kind=kind)):
                    continue
                kw = dict(L=L, node_type=nt, quant=quant_for(kind, N))
                if kind == "CA-SCL":
                    crc_n = 24 if K >= 64 else 11
                    kw.update(A=K - crc_n, crc_n=crc_n, crc_loc=S.CRC24_LOC if crc_n == 24 else S.CRC11_LOC)
                want = oracle_mod.decode_float(kind, N, K, fm, llr, **kw)
                got = oracle_mod.decode_float_status(kind, N, K, fm, llr, **kw)
                assert (got[0] == want).all(), (kind, N, K, L, style)


# -- against the restatement of the reference's walk ----------------------------------------------------------

# N, K, A, crc_n, Eb/N0: one code per N; CRC11 where 24 check bits do not fit, and at N = 256; (1024, 500, 512)
# compares K - A = 12 of the 24 check bits
REF_CODES = [(8, 6, 2, 11, 3.0), (32, 30, 6, 24, 3.0), (128, 64, 40, 24, 1.0), (256, 111, 100, 11, 1.5),
             (1024, 512, 500, 24, 1.5)]


@pytest.mark.parametrize("tables", ["random", "continuous", "minsum"])
@pytest.mark.parametrize("N,K,A,crc_n,ebn0", REF_CODES)
def test_status_matches_restatement(N, K, A, crc_n, ebn0, tables, oracle_mod):
    """One walk of status_ref per (code, L, tables) on CRC-carrying frames; its paths and metrics then go
    through both output stages: SCL-LUT's first minimum, and CA-SCL-LUT's CRC walk under each mask."""
    for L in (2, 3, 5, 8):
        c = S.Case("CA-SCL-LUT", N, K, L, tables, A=A, crc_n=crc_n, ebn0=ebn0, B=24 if N == 1024 else 96)
        fm, nt, _ = S.code_of(c)
        p, x = S.tables_of(c), S.inputs_of(c)
        walked = [status_ref._decode_frame(p, np.asarray(fm), L, y) for y in x]
        want = status_ref.select(walked, None)
        assert same(oracle_mod.decode_lut_status("SCL-LUT", p, K, L, fm, x), want), (L, "no CRC")
        for mb in sorted({0, 1, min(16, crc_n), crc_n}):
            mask = S.crc_mask(mb) if mb else None
            want = status_ref.select(walked, A, crc_n, c.crc_loc, mask)
            got = oracle_mod.decode_lut_status("CA-SCL-LUT", p, K, L, fm, x, A=A, crc_n=crc_n, crc_loc=c.crc_loc, mask=mask)
            assert same(got, want), (L, mb)


def test_status_matches_restatement_on_random_symbols(oracle_mod):
    """The sweep's frames without a CRC are random symbols, not codewords in noise: the restatement's own
    decode() on the inputs of one such sweep case per table kind."""
    for tables in ("random", "continuous", "minsum"):
        c = S.Case("SCL-LUT", 64, 20, 5, tables)
        assert c in S.CASES
        fm, nt, _ = S.code_of(c)
        x, ref = S.reference(c)
        assert same(ref[0], status_ref.decode(S.tables_of(c), np.asarray(fm), c.L, x)), tables


# -- against the reference's recorded status ------------------------------------------------------------------

@pytest.mark.parametrize("path", BD_FILES, ids=lambda p: os.path.basename(p)[:-4])
def test_status_matches_reference_bd(path, oracle_mod):
    g = load_golden(path)
    N, K, L, A = int(g["N"]), int(g["K"]), int(g["L"]), int(g["A"])
    for mask, idx in bd_groups(g):
        bits, pml, win, ok = oracle_mod.decode_float_status("CA-SCL", N, K, g["frozen"], g["llr"][idx], L=L, A=A,
                                                            crc_n=int(g["crc_n"]), crc_loc=g["crc_loc"], mask=mask)
        assert (bits == g["bits"][idx]).all() and (ok == g["is_pass"][idx]).all()
        # the reference returns PML[i], i the winner's rank in its argsort (the deviation of include/qpd.h).
        # The rank lies between the count of smaller metrics and that of smaller-or-equal ones less one,
        # wherever the sort put the equal ones; on these codes (the last position an information bit) the
        # final metrics ascend with the path index, so every PML[i] in that range is one and the same double
        f = np.arange(len(idx))
        own = pml[f, win]
        lo, hi = (pml < own[:, None]).sum(1), (pml <= own[:, None]).sum(1) - 1
        assert g["frozen"][-1] == 0 and (np.diff(pml, axis=1) >= 0).all()
        assert (pml[f, lo] == g["pm"][idx]).all() and (pml[f, hi] == g["pm"][idx]).all()
        # what the library documents: the output path's own metric
        assert (own == g["pm"][idx]).all()


# -- against the host engine ----------------------------------------------------------------------------------

def host_decoder(c):
    from quantized_decoder_polar_codes_amd import decoders as D

    fm, nt, _ = S.code_of(c)
    kw = dict(A=c.A, crc_n=c.crc_n, crc_loc=c.crc_loc) if c.A else {}
    if c.is_float:
        return D.from_quant(c.kind, c.N, c.K, fm, L=c.L, node_type=nt, quant=S.quant_of(c), create=False, **kw)
    return D.from_packed(c.kind, S.tables_of(c), c.K, fm, L=c.L, node_type=nt, create=False, **kw)


@pytest.mark.parametrize("c", REF_KEYS, ids=lambda c: c.id)
def test_status_matches_host_engine(c, harness):
    x, ref = S.reference(c)
    dec = host_decoder(c)
    for mb, want in ref.items():
        rc, bits, m, ok = host_status(harness, dec, x, mask=S.crc_mask(mb) if mb else None, crc_pass=bool(c.A))
        if c.kind in ("SCL-Uniform", "SCL-Lloyd"):  # not the host engine's (include/qpd.h, qpd_set_host_engine)
            assert rc == QPD_E_UNSUPPORTED  # no second implementation: the metric rests on the oracle alone
            return
        assert rc == 0, c.id
        assert (bits == want[0]).all(), (c.id, mb)
        assert (m == want[1][np.arange(len(x)), want[2]]).all(), (c.id, mb)
        if c.A:
            assert (ok == want[3]).all(), (c.id, mb)


# -- the sweep's own premises ---------------------------------------------------------------------------------

@pytest.mark.parametrize("c", [c for c in {c.ref_key(): c for c in S.CASES}.values() if c.B > 1], ids=lambda c: c.id)
def test_sweep_case_is_informative(c):
    S.check_informative(c)


def test_unmet_conditions_cannot_be_met(oracle_mod):
    """The reasons of status_cases.UNMET, shown: of all 16^4 inputs of the (4, 2, 2) min-sum cases none ends
    with two equal metrics.  (That random tables pass no CRC is asserted per case: no mask changes a frame.)"""
    import itertools

    x = np.array(list(itertools.product(range(16), repeat=4)), dtype=np.int32)
    for c in S.CASES:
        if "ties" in c.unmet:
            assert (c.L, c.tables) == (2, "minsum")
            assert S.informative_counts(c)[0] == 0  # else the condition can be met: assert it
        if "ties" in c.unmet and c.N == 4:
            fm, nt, _ = S.code_of(c)
            _, pml, _, _ = oracle_mod.decode_lut_status(c.kind, S.tables_of(c), c.K, c.L, fm, x, node_type=nt)
            assert (pml[:, 0] != pml[:, 1]).all()


def planned(c, ph):
    """(engine, lanes_per_frame, frames_per_wave, fast_variant, prefix_ops > 0) of qpd_info as the host-only
    planner decides them: the generic engine's lane groups (plan_generic), the fast engine's plan_fast."""
    gs = 1
    while gs < c.L:
        gs *= 2
    if c.is_float or c.engine == "generic":
        return (S.GENERIC, gs, 64 // gs, 0, False)
    env = dict(c.env)
    sw = {name.lower()[4:]: True for name in ("QPD_NO_PFX", "QPD_NO_PRE", "QPD_PFX1B", "QPD_NO_PW1") if name in env}
    for name in ("QPD_SETS", "QPD_LDS_BUDGET", "QPD_PRE_CHUNK"):
        if name in env:
            sw[name.lower()[4:]] = int(env[name])
    rc, msg, st = TP.check(ph, host_decoder(c), TP.switches(**sw))
    scl = c.kind in ("SCL-LUT", "CA-SCL-LUT")
    if c.engine == "auto" and (rc == -100 or c.L > (16 if scl else 8)):  # include/qpd.h, enum qpd_engine
        return (S.GENERIC, gs, 64 // gs, 0, False)
    assert rc == 0, (c.id, rc, msg)
    return (S.FAST, gs, 64 // gs * int(st["sets"]), int(st["pw1"]) | 2 * int(st["r1l"]), bool(st["pfx_ops"] > 0))


@pytest.mark.parametrize("c", S.CASES, ids=lambda c: c.id)
def test_sweep_case_reaches_its_instantiation(c, plan_harness):
    assert planned(c, plan_harness) == S.EXPECT[c.id]


def test_expect_lists_the_sweep():
    assert list(S.EXPECT) == [c.id for c in S.CASES]


def test_sweep_reaches_every_status_kernel():
    """Every selector of the *_st.hip units (qpd_capi_build.hpp: fast_kernel) has a case: unit by kind family,
    pointer words and list width, then frame sets, l8 and (FastSCL-LUT) r1l; and the generic status tail on the
    LUT and float domains with narrow (<= 8) and wide lists."""
    fast, generic = set(), set()
    for c in S.CASES:
        eng, gs, fpw, variant, _ = S.EXPECT[c.id]
        fam = "fscl" if "Fast" in c.kind else "scl"
        if eng == S.FAST:
            fast.add((fam, c.L > 8, bool(variant & 1), fpw * gs // 64, c.L == 8, bool(variant & 2)))
        else:
            generic.add(("float" if c.is_float else "lut", c.L > 8))
    assert generic == {(d, w) for d in ("lut", "float") for w in (False, True)}
    units = {(fam, w16, pw1) for fam, w16, pw1, *_ in fast}
    assert units >= {("scl", False, False), ("scl", False, True), ("scl", True, False), ("scl", True, True),
                     ("fscl", False, False), ("fscl", False, True), ("fscl", True, False), ("fscl", True, True)}
    both = (False, True)
    # the selector arguments jointly: fast_kernel_scl*_st(sets, l8, w16), fast_kernel_fscl_st(sets, l8, r1l),
    # fast_kernel_fscl_w16_st(sets, pw1); fast_kernel_fscl_pw1_st has (2, l8, no r1l) alone
    assert {(sets, l8) for f, w16, _, sets, l8, _ in fast if f == "scl" and not w16} == {(s, b) for s in (1, 2) for b in both}
    assert {(sets, l8, r1l) for f, w16, pw1, sets, l8, r1l in fast if f == "fscl" and not w16 and not pw1} \
        == {(s, b, r) for s in (1, 2) for b in both for r in both}
    assert {(sets, l8, r1l) for f, w16, pw1, sets, l8, r1l in fast if f == "fscl" and not w16 and pw1} == {(2, True, False)}
    for fam in ("scl", "fscl"):
        assert {sets for f, w16, _, sets, _, _ in fast if f == fam and w16} == {1, 2}
    assert {(sets, pw1) for f, w16, pw1, sets, _, _ in fast if f == "fscl" and w16} == {(s, b) for s in (1, 2) for b in both}
