"""The fast engine's table lookups and f / g ops, called directly on the device.

Every decode on the fast engine spends most of its time in qpd_fast_lookup.hpp: the
nibble-table lookups (lut4, lut_vec, lut_byte, stage_tab + lut_lds), the SWAR helpers around
them, the channel readers, and the ops built from them (fg_op, fg_chan_op, ff_op, gsel_op;
root_pre_kernel in qpd_fast_pre.hpp).  A decode reaches only the (element position, a, b, u)
combinations its tables and frames happen to produce; the harness
(tests/native/lookup_harness.hip) hands chosen operands, tables and rows to these functions
themselves.  The inputs come from tests/lookup_cases.py, whose generators assert that every
cell of each function's domain is covered; the expected results from tests/lookup_ref.py,
plain numpy that tests/test_lookup_cases.py pins to the reference decoder.

All comparisons are exact.  Every case asserts the harness's canaries; every op case checks
the whole LDS and slab images: the destination rows in full (64 lanes, every set), every
other row unchanged.  The harness is built three times (QPD_VEC_CHAIN 0 / 1, QPD_GSWZ = 72);
the functions a switch changes run on the variants that differ.
"""
import numpy as np
import pytest

import lookup_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def harnesses(native_lib):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import lookup_harness as LH

    hs = {v: LH.load(v) for v in LH.VARIANTS}  # rebuilt only when the harness or csrc/ changed
    assert (hs["chain0"].vec_chain, hs["chain1"].vec_chain, hs["gswz72"].gswz) == (0, 1, 72)
    assert all(h.lutmask == 0xFFFF for h in hs.values())
    return LH, hs


def _table_sets(v):
    return C.table_sets(v, 7000 + v).items()


def _check_lookup(h, fn, tsel, case, v, tf, tg, what):
    got = h.prim(fn, tsel, v, tf, tg, case["A"], case["B"], case["H"])
    want = C.lookup_expected(case, tf[0], tg, v)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} lanes differ; first lane {bad[0]}: A={case['A'][bad[0]]:#x} "
                           f"B={case['B'][bad[0]]:#x} H={case['H'][bad[0]]:#x} got {got[bad[0]]:#x} want {want[bad[0]]:#x}")


# -- primitives --------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["chain0", "chain1"])
@pytest.mark.parametrize("v", C.LOOKUP_V)
def test_lut_vec(harnesses, variant, v):
    """lut4 and lut_vec<2|4|8>, lut_vec<8, IL>: every (k, a * 16 + b, half), garbage above the elements."""
    LH, hs = harnesses
    h = hs[variant]
    rng = np.random.default_rng(v)
    for name, (tf, tg) in _table_sets(v):
        _check_lookup(h, LH.LUT4, LH.T_G, C.lut4_case(v, rng), v, tf, tg, f"lut4 {name}")
        for fn, ne, il in ((LH.VEC2, 2, False), (LH.VEC4, 4, False), (LH.VEC8, 8, False), (LH.VEC8IL, 8, True)):
            for isg in (False, True):
                _check_lookup(h, fn, LH.T_G if isg else LH.T_F, C.vec_case(ne, v, isg, il, rng), v, tf, tg,
                              f"lut_vec<{ne}, il={il}> g={isg} {name} v={v}")


@pytest.mark.parametrize("v", C.LOOKUP_V)
def test_lut_byte(harnesses, v):
    """The four forms bot3_op uses; W's bytes above NE - 1 and H outside bit 8 k + 7 are garbage."""
    LH, hs = harnesses
    rng = np.random.default_rng(50 + v)
    for name, (tf, tg) in _table_sets(v):
        for fn, ne, il, has_h in ((LH.BYTE2, 2, False, False), (LH.BYTE2H, 2, False, True), (LH.BYTE4, 4, True, False),
                                  (LH.BYTE4H, 4, True, True)):
            _check_lookup(hs["chain0"], fn, LH.T_G if has_h else LH.T_F, C.byte_case(ne, v, has_h, il, rng), v, tf, tg,
                          f"lut_byte<{ne}, {il}, {has_h}> {name} v={v}")
        # the second of two packed f tables (Tf12 with H = 0x8080): the upper half is node 1's f table
        case = C.byte_case(2, v, True, False, rng)
        both = np.stack([tf[0], tf[1]])
        got = hs["chain0"].prim(LH.BYTE2H, LH.T_FF, v, tf, tg, case["A"], case["B"], case["H"])
        assert np.array_equal(got, C.lookup_expected(case, None, both, v)), f"lut_byte<2> on two f tables {name} v={v}"


@pytest.mark.parametrize("variant", ["chain0", "gswz72"])
@pytest.mark.parametrize("v", C.LOOKUP_V)
def test_stage_tab_lut_lds(harnesses, variant, v):
    """stage_tab then lut_lds<8, false>, <8, true>, <8, true, 0, true> and <8, false, 512>."""
    LH, hs = harnesses
    rng = np.random.default_rng(90 + v)
    for name, (tf, tg) in _table_sets(v):
        for fn, isg, il in ((LH.LDS8F, False, False), (LH.LDS8G, True, False), (LH.LDS8GIL, True, True),
                            (LH.LDS8F512, False, False)):
            _check_lookup(hs[variant], fn, LH.T_G if isg else LH.T_F, C.vec_case(8, v, isg, il, rng), v, tf, tg,
                          f"lut_lds fn {fn} {name} v={v} {variant}")


def test_bit_helpers(harnesses):
    LH, hs = harnesses
    tf, tg = C.index_tables(16)
    fns = {"nib_interleave8": LH.INTERLEAVE, "il_nib": LH.ILNIB, "half_bits2": LH.HALF2, "half_bits4": LH.HALF4,
           "nib_pack4": LH.PACK4, "nib2byte4": LH.N2B4, "nib_mask": LH.NIBMASK, "polar_word": LH.POLAR}
    cases = C.helper_cases(np.random.default_rng(11))
    assert set(cases) == set(fns)
    for name, (x, want) in cases.items():
        got = hs["chain0"].prim(fns[name], LH.T_F, 16, tf, tg, x)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{name}: {bad.size} inputs differ; first {x[bad[0]]:#x}: got {got[bad[0]]:#x} want {want[bad[0]]:#x}"


@pytest.mark.parametrize("v", C.CHAN_V)
def test_channel_readers(harnesses, v):
    """Every byte value (int32: also -1, 2^31 - 1, high bits only) at each of the 8 positions: bad symbols read
    as 0 and raise the error word of exactly the lanes whose word holds one."""
    LH, hs = harnesses
    h = hs["chain0"]
    rng = np.random.default_rng(300 + v)
    runs = [(LH.W8_I32_VEC, False, 0, False), (LH.W8_I32_VEC, False, 4, False), (LH.W8_I32, False, 0, False),
            (LH.W8_I32, False, 3, False), (LH.W8_U8_VEC, True, 0, False), (LH.W8_U8_VEC, True, 8, False),
            (LH.W8_U8, True, 0, False), (LH.W8_U8, True, 5, False), (LH.WORD_I32, False, 1, True),
            (LH.WORD_U8, True, 3, True), (LH.SMALL, False, 1, True)]
    for mode, u8, base, counted in runs:
        c = C.chan_case(u8, v, base, rng, counted=counted)
        word, err = h.chan(mode, v, c["buf"], c["e0"], c["cnt"])
        assert np.array_equal(word, c["word"]), f"reader {mode} base {base} v={v}: {int((word != c['word']).sum())} words differ"
        assert np.array_equal(err, c["err"]), f"reader {mode} base {base} v={v}: {int((err != c['err']).sum())} error words differ"


# -- ops ---------------------------------------------------------------------------------------------
def _run_op(LH, h, kind_id, case, tf, tg, lt=False, what=""):
    rc, lds, slab, err, ok = h.op_raw(kind_id, case["isg"], lt, case["pre"], case["cnt"], case["v"], case["in_vec"], case["gs"],
                                      case["spaces"], case["rows"], tf, tg, case["y"], case["lds"], case["slab"], case["srcf"],
                                      case["usrcf"])
    assert rc == 0, f"{what}: error {rc}"
    assert (ok == 3).all(), f"{what}: canaries / read rows of blocks {np.flatnonzero(ok != 3)}: {ok}"
    for name, got, want in (("LDS", lds, case["exp_lds"]), ("slab", slab, case["exp_slab"])):
        bad = np.argwhere(got != want)  # [block, row, set, lane]
        assert bad.size == 0, (f"{what}: {len(bad)} {name} words differ; first (block, row, set, lane) {bad[0]}: got "
                               f"{got[tuple(bad[0])]:#x} want {want[tuple(bad[0])]:#x}; rows {case['rows']}")
    assert np.array_equal(err, case["exp_err"]), f"{what}: error words {err}, expected {case['exp_err']}"


def _g_modes():  # (isg, U rows in LDS)
    return [(False, False), (True, False), (True, True)]


@pytest.mark.parametrize("variant,lt", [("chain0", False), ("chain1", False), ("chain0", True), ("gswz72", True)])
@pytest.mark.parametrize("ns", [1, 2])
def test_fg_op_rows(harnesses, variant, lt, ns):
    """fg_op<ISG, true, NS, SL, DL, LT>: slab -> slab, slab -> LDS, LDS -> LDS; U rows in either space."""
    LH, hs = harnesses
    rng = np.random.default_rng(17 * ns + lt)
    for v in (16, 3):
        tf, tg = C.random_tables(v, rng)
        for cnt in (8, 16, 32, 64, 128, 256):
            for place in (0, LH.DST_LDS, LH.SRC_LDS | LH.DST_LDS):
                for isg, ul in _g_modes():
                    case = C.op_case("fg", isg, cnt, v, ns, 8, place | (LH.U_LDS if ul else 0), tf, tg, rng)
                    _run_op(LH, hs[variant], LH.K_FG, case, tf, tg, lt,
                            f"fg_op g={isg} cnt={cnt} ns={ns} spaces={case['spaces']} lt={lt} v={v} {variant}")


@pytest.mark.parametrize("ns", [1, 2])
def test_fg_op_small_and_pre(harnesses, ns):
    """fg_op<ISG, false>: the one-word forms cnt 2 / 4 from a row, and MF_PRE rows for cnt >= 8."""
    LH, hs = harnesses
    rng = np.random.default_rng(40 + ns)
    tf, tg = C.random_tables(16, rng)
    for variant in ("chain0", "chain1"):
        for isg, ul in _g_modes():
            for cnt in (2, 4):
                for place in (0, LH.DST_LDS, LH.SRC_LDS | LH.DST_LDS):
                    for gs in (8, 16):
                        case = C.op_case("fgp", isg, cnt, 16, ns, gs, place | (LH.U_LDS if ul else 0), tf, tg, rng)
                        _run_op(LH, hs[variant], LH.K_FGP, case, tf, tg, what=f"fg_op<., false> g={isg} cnt={cnt} ns={ns} gs={gs}")
            for cnt in (8, 16, 32, 64, 128, 256):
                for place in (0, LH.DST_LDS):
                    case = C.op_case("fgp", isg, cnt, 16, ns, 8, place | (LH.U_LDS if ul else 0), tf, tg, rng, pre=True)
                    _run_op(LH, hs[variant], LH.K_FGP, case, tf, tg, what=f"fg_op<., false> MF_PRE g={isg} cnt={cnt} ns={ns}")


@pytest.mark.parametrize("ns", [1, 2])
def test_fg_chan_op(harnesses, ns):
    """fg_chan_op on int32 channel rows, in_vec on and off; one case with out-of-range symbols."""
    LH, hs = harnesses
    rng = np.random.default_rng(60 + ns)
    for v in (16, 3):
        tf, tg = C.random_tables(v, rng)
        for isg, ul in _g_modes():
            for cnt in (2, 4, 8, 64):
                for in_vec in (False, True):
                    for bad in (False, True):
                        case = C.op_case("chan", isg, cnt, v, ns, 8, (LH.DST_LDS if cnt < 64 else 0) | (LH.U_LDS if ul else 0),
                                         tf, tg, rng, in_vec=in_vec, bad_symbols=bad)
                        _run_op(LH, hs["chain0"], LH.K_CHAN, case, tf, tg,
                                what=f"fg_chan_op g={isg} cnt={cnt} ns={ns} in_vec={in_vec} bad={bad} v={v}")


@pytest.mark.parametrize("variant", ["chain0", "gswz72"])
@pytest.mark.parametrize("ns", [1, 2])
def test_ff_op(harnesses, variant, ns):
    """ff_op: S[d + 1] at dst_row and S[d + 2] at r_row, the tables staged at tb and tb + 512."""
    LH, hs = harnesses
    rng = np.random.default_rng(80 + ns)
    for v in (16, 3):
        tf, tg = C.closed_tables(v, rng)  # the child's f looks the op's results up: symbols of the alphabet
        for cnt in (32, 64, 256):
            for place in (0, LH.CHILD_LDS, LH.DST_LDS | LH.CHILD_LDS):
                for isg, ul in _g_modes():
                    case = C.op_case("ff", isg, cnt, v, ns, 8, place | (LH.U_LDS if ul else 0), tf, tg, rng)
                    _run_op(LH, hs[variant], LH.K_FF, case, tf, tg, what=f"ff_op g={isg} cnt={cnt} ns={ns} spaces={case['spaces']} v={v}")


@pytest.mark.parametrize("ns", [1, 2])
def test_gsel_op(harnesses, ns):
    """gsel_op on nwo = 1, 2, 4, 8, 16, 32 words.  plan_fast emits MF_GSEL only at the root in pre-mode with
    op.cnt = N / 2 and N = 2^n >= 16 (fast_ops in qpd_plan.hpp: m.cnt = N >> (d + 1) at d = 0), so op.cnt is a
    power of two from 8 on: cnt = 40 (nwo = 5) and every other nwo in 5..7 cannot be emitted.  nwo = 8 (cnt =
    64) is the first with the second u word, 16 and 32 run the chunk loop more than once."""
    LH, hs = harnesses
    rng = np.random.default_rng(120 + ns)
    tf, tg = C.random_tables(16, rng)
    for cnt in (8, 16, 32, 64, 128, 256):
        for place in (0, LH.DST_LDS, LH.U_LDS, LH.DST_LDS | LH.U_LDS):
            for gs in (8, 4):
                case = C.op_case("gsel", True, cnt, 16, ns, gs, place, tf, tg, rng)
                _run_op(LH, hs["chain0"], LH.K_GSEL, case, tf, tg, what=f"gsel_op cnt={cnt} ns={ns} spaces={place} gs={gs}")


@pytest.mark.parametrize("u8", [False, True])
def test_root_pre_kernel(harnesses, u8):
    """root_pre_kernel: B << (n - 4) no multiple of 256, one block (the grid-stride loop) and three (the
    clamped tail thread); nothing outside [f | g0 | g1] of each row changes, nor the row after the last."""
    LH, hs = harnesses
    rng = np.random.default_rng(140 + u8)
    for v in (16, 3):
        tf, tg = C.random_tables(v, rng)
        for n, B in ((4, 700), (5, 333), (10, 9)):
            assert (B << (n - 4)) % 256 != 0
            for grid in (1, 3):
                for in_vec, in_off in ((True, 0), (True, 8), (False, 0), (False, 3)):
                    for bad in (False, True):
                        c = C.root_pre_case(u8, n, B, v, in_off, tf, tg, rng, bad_symbols=bad)
                        rc, pre, err = hs["chain0"].root_pre_raw(u8, n, v, grid, in_vec, in_off, tf, tg, c["inp"], c["pre"])
                        what = f"root_pre u8={u8} N={1 << n} B={B} grid={grid} in_vec={in_vec} off={in_off} bad={bad} v={v}"
                        assert rc == 0, f"{what}: error {rc}"
                        diff = np.flatnonzero(pre != c["exp"])
                        assert diff.size == 0, f"{what}: {diff.size} words differ, first word {diff[0]} (row {diff[0] // (1 << n - 2)})"
                        assert err == c["err"], f"{what}: error word {err}"


def test_entry_points_refuse_what_the_kernels_cannot_run(harnesses):
    LH, hs = harnesses
    h = hs["chain0"]
    rng = np.random.default_rng(9)
    tf, tg = C.random_tables(16, rng)
    z = np.zeros(64, np.uint32)
    assert h.prim_raw(LH.VEC8, LH.T_G, 16, tf, tg, z[:63])[0] == -1        # not whole waves
    assert h.prim_raw(LH.LUT4, LH.T_G, 16, tf, tg, z, z + 512)[0] == -1    # an index past the table
    assert h.prim_raw(LH.LDS8G, LH.T_F, 16, tf, tg, z)[0] == -1            # g lookups on an f table
    assert h.prim_raw(99, LH.T_F, 16, tf, tg, z)[0] == -1
    buf = np.zeros(64 * 8, np.int32)
    e0 = (8 * np.arange(64)).astype(np.int32)
    assert h.chan_raw(LH.W8_I32, 16, buf, e0 + 1, np.full(64, 8))[0] == -1       # past the buffer
    assert h.chan_raw(LH.W8_I32_VEC, 16, np.zeros(64 * 8 + 8, np.int32), e0 + 1, np.full(64, 8))[0] == -1  # unaligned
    assert h.chan_raw(LH.W8_I32, 17, buf, e0, np.full(64, 8))[0] == -1
    case = C.op_case("fg", True, 64, 16, 2, 8, LH.DST_LDS, tf, tg, rng)

    def op(**kw):
        a = dict(case, **kw)
        return h.op_raw(kw.get("kind_id", LH.K_FG), a["isg"], False, a["pre"], a["cnt"], a["v"], a["in_vec"], a["gs"], a["spaces"],
                        a["rows"], tf, tg, a["y"], a["lds"], a["slab"], a["srcf"], a["usrcf"])[0]

    assert op() == 0
    assert op(spaces=LH.SRC_LDS) == -1                                   # LDS -> slab: the planner refuses it
    assert op(rows=case["rows"] + np.array([0, 1000, 0, 0], np.int32)) == -1  # a destination past the LDS rows
    assert op(rows=case["rows"] + np.array([1000, 0, 0, 0], np.int32)) == -1
    assert op(cnt=48) == -1
    assert op(srcf=case["srcf"] + 8) == -1                               # a slot outside the lane's group
    assert op(kind_id=LH.K_FF, spaces=LH.DST_LDS) == -1                  # S[d + 2] in the slab below S[d + 1] in LDS
