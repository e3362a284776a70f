"""The fast engine's plan compiler (csrc/qpd_plan.hpp) checked on the CPU.

The plan decides every LDS and slab row the kernels of qpd_fast.hip touch; a
wrong row there is silent corruption or a memory fault, not a failed assert.
tests/native/plan_harness.cpp (g++, no HIP) plans a configuration the way
qpd_create does and verifies in C++ what the kernels rely on: rows inside
their space and in slots the layout kept, the R1 argsort scratch, the LDS
size and budget, the pointer fields and every other value packed into part of a
record word (read back by the kernels' own expressions), the prefix stages' records, the
f / g shape plan_fast refuses, and that planning twice gives the same bytes.

The sweep: every LUT kind; the 5G PW codes at N = 8 .. 1024 with a low, half
and high rate, N = 2048 and 4096 with the BEC construction (N = 8192, 16384 and 65536
under a reduced switch list); L = 1 (SC kinds) or
2, 4, 8, 12, 16; tie-heavy random tables and the MinDistortion tables of the
committed goldens; each switch on its own and the LDS budgets the GPU tests use.
Beside that point of the input space (v = 16, nested reliability orders): the
alphabets 2, 3, 8 and 15, and the random, block-structured and edge masks of
tests/code_masks.py at N = 8 .. 1024.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import code_masks as M
from conftest import ROOT, GOLDEN_DIR, golden_packed, load_golden

CSRC = os.path.join(ROOT, "quantized_decoder_polar_codes_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")
KINDS = ["SC-LUT", "SCL-LUT", "FastSC-LUT", "FastSCL-LUT"]
UNSET = -2 ** 31
E_UNSUPPORTED = -2
W16_REFUSAL = ("fast engine, FastSCL-LUT with L > 8: an R1 node of more than 32 elements, or of more than 16 "
               "without room for its argsort in LDS, is not served (use the generic engine)")
MF_VUNI, MF_BOTX, MF_R1_RK, MF_SFG = 8192, 33554432, 67108864, 134217728


class Switches(ctypes.Structure):
    """qpd_plan::PlanSwitches (a non-diagnostic build)."""
    _fields_ = [("sets", ctypes.c_int), ("lds_budget", ctypes.c_int), ("pre_chunk", ctypes.c_int64),
                ("pfx_sets", ctypes.c_int)] + [(f, ctypes.c_bool) for f in (
                    "pfx1b", "no_pre", "no_bfuse", "no_botx", "no_trim", "no_pfx", "no_pfx2", "no_ff", "no_bc2", "no_pw1",
                    "no_vuni", "no_r1rk", "no_sfold")]


def switches(**kw):
    return Switches(**{"lds_budget": UNSET, **kw})


# default, each switch on its own (the values the GPU tests use), the LDS budgets
SWEEP = ([{}, {"sets": 1}, {"sets": 2}, {"pre_chunk": 7}, {"pfx_sets": 1}]
         + [{f: True} for f, _ in Switches._fields_[4:]]
         + [{"lds_budget": b} for b in (256, 2048, 4096, 10240, 65536)])


def load_harness():
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "plan_harness.so")
    src = os.path.join(ROOT, "tests", "native", "plan_harness.cpp")
    deps = [src] + [os.path.join(CSRC, f) for f in ("qpd_plan.hpp", "qpd_mop.hpp", "qpd_schedule.hpp", "qpd_types.hpp",
                                                    "stl_sort.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                        src, "-o", so + ".tmp"], check=True)
        os.replace(so + ".tmp", so)
    L = ctypes.CDLL(so)
    L.ph_check.argtypes = [ctypes.c_void_p, ctypes.POINTER(Switches), ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p]
    L.ph_check.restype = ctypes.c_int
    L.ph_switches_size.restype = ctypes.c_int
    assert L.ph_switches_size() == ctypes.sizeof(Switches)
    return L


@pytest.fixture(scope="module")
def harness():
    return load_harness()


def check(harness, dec, sw):
    """(return code, message, stats) of one planned configuration."""
    msg = ctypes.create_string_buffer(512)
    stats = np.zeros(8, dtype=np.int32)
    rc = harness.ph_check(ctypes.byref(dec._cfg), ctypes.byref(sw), msg, len(msg), stats.ctypes.data)
    return rc, msg.value.decode(), dict(zip(("lds_from", "nops", "pfx_ops", "pw1", "r1l", "flags", "sets", "w16"), stats))


def code(N, K):
    from quantized_decoder_polar_codes_amd import codes as C

    if N <= 1024:
        _, mb, fm, mm = C.construct_pw(N, K)
    else:  # beyond the 5G sequence: BEC(1/2) Bhattacharyya construction (tests/test_gpu_schedule_modes.py)
        z = np.array([0.5])
        while z.size < N:
            z = np.stack([2 * z - z * z, z * z], axis=1).reshape(-1)
        fm = np.zeros(N, dtype=np.int64)
        fm[np.argsort(-z, kind="stable")[: N - K]] = 1
        mb = np.flatnonzero(fm == 0)
    return fm, C.identify_nodes(N, mb).astype(np.int32)


def r1_sizes(nt, N):
    """Sizes of the R1 nodes a FastSCL-LUT schedule visits (labels 0 / 1 / 2 = R0 / R1 / REP end the descent)."""
    out, stack = [], [(0, 0)]
    while stack:
        d, node = stack.pop()
        t = nt[(1 << d) + node - 1]
        if 0 <= t <= 2:
            if t == 1:
                out.append(N >> d)
        elif (2 << d) < N:
            stack += [(d + 1, 2 * node), (d + 1, 2 * node + 1)]
    return out


def rates(N):
    return sorted({max(1, N // 4), N // 2, 3 * N // 4})


def sweep(harness, kind, N, K, packed, Ls, sweep_switches, fm=None):
    """Plans (kind, N, K) for every L and switch setting; the refusals as {(L, switch setting)}.  `fm`: a
    frozen mask with K zeros to plan instead of the reliability order's."""
    from quantized_decoder_polar_codes_amd import decoders as D

    if fm is None:
        fm, nt = code(N, K)
    else:
        nt = M.node_type_of(fm)
    if kind.startswith("Fast") and 0 <= nt[0] <= (3 if kind == "FastSC-LUT" else 2):
        return None  # a special root is rejected by qpd_create's validation, before any plan
    refused, seen = set(), 0
    for L in Ls:
        dec = D.from_packed(kind, packed, K, fm, L=L, node_type=nt, create=False)
        for kw in sweep_switches:
            rc, msg, st = check(harness, dec, switches(**kw))
            where = f"{kind} N={N} K={K} L={L} switches={kw}"
            assert rc != -100, f"{where}: not a fast-engine configuration"
            if rc < 0:
                # the one refusal of the sweep: FastSCL-LUT on the W16 plan with an R1 node it cannot serve
                big = r1_sizes(nt, N)
                assert (rc, msg) == (E_UNSUPPORTED, W16_REFUSAL) and kind == "FastSCL-LUT" and L > 8 and max(big, default=0) > 16, \
                    f"{where}: refused with {rc}: {msg}"
                refused.add((L, tuple(kw.items())))
                continue
            assert rc == 0, f"{where}: {msg}"
            if kind == "FastSCL-LUT" and L > 8:  # R1 nodes above 32 elements are never served there
                assert max(r1_sizes(nt, N), default=0) <= 32, f"{where}: planned with an R1 node of > 32 elements"
            seen |= int(st["flags"])
    return refused, seen


def list_sizes(kind):
    return [2, 4, 8, 12, 16] if "SCL" in kind else [1]


@pytest.mark.parametrize("N", [8, 16, 32, 64, 128, 256, 512, 1024])
@pytest.mark.parametrize("kind", KINDS)
def test_plan_invariants_random_tables(kind, N, harness):
    from quantized_decoder_polar_codes_amd import lut as LU

    p = LU.random_luts(N, 16, seed=3 * N + 1, distinct_mags=3)
    for K in rates(N):
        sweep(harness, kind, N, K, p, list_sizes(kind), SWEEP)


@pytest.mark.parametrize("v", [2, 3, 8, 15])
@pytest.mark.parametrize("N", [8, 16, 32, 64, 128, 256, 512, 1024])
@pytest.mark.parametrize("kind", KINDS)
def test_plan_invariants_alphabets(kind, N, v, harness):
    """Alphabets below 16 on the reliability order, per-element quanta and (node_rows) one row per node."""
    from quantized_decoder_polar_codes_amd import lut as LU

    seen = 0
    for node_rows in (False, True):
        p = LU.random_luts(N, v, seed=3 * N + v, distinct_mags=3, node_rows=node_rows)
        for K in rates(N):
            r = sweep(harness, kind, N, K, p, list_sizes(kind), SWEEP)
            if r is not None:
                seen |= r[1]
    if kind.startswith("Fast") and N >= 64:
        assert seen & MF_VUNI


def mask_cases(N):
    """(name, mask) of the three mask families at N."""
    out = [(f"random{s}", M.random_mask(N, K, s)) for s, K in enumerate(rates(N))]
    out += [(f"block{s}", M.block_mask(N, s)) for s in M.BLOCK_SEEDS.get(N, (3, 4, 5))]
    return out + list(M.edge_masks(N).items())


@pytest.mark.parametrize("v", [16, 8])
@pytest.mark.parametrize("N", [8, 16, 32, 64, 128, 256, 512, 1024])
@pytest.mark.parametrize("kind", KINDS)
def test_plan_invariants_masks(kind, N, v, harness):
    """Masks no reliability order gives: an empty frozen prefix, a frozen last position, R1 before R0, special
    nodes of every size in any order.  The only refusal stays the W16 one (sweep asserts it)."""
    from quantized_decoder_polar_codes_amd import lut as LU

    p = LU.random_luts(N, v, seed=5 * N + v, distinct_mags=3, node_rows=True)
    unplanned = set()
    for name, fm in mask_cases(N):
        r = sweep(harness, kind, N, int((fm == 0).sum()), p, list_sizes(kind), SWEEP, fm=fm)
        assert (r is None) == M.special_root(fm, kind), name
        if r is None:
            unplanned.add(name)
    if N >= 16:  # a special root, which qpd_create's validation rejects: all_info alone (at N = 8 a block mask may be one node)
        assert unplanned == ({"all_info"} if kind.startswith("Fast") else set())


@pytest.mark.parametrize("N,K", [(2048, 512), (2048, 1024), (2048, 1536), (4096, 1400), (4096, 2048), (4096, 3072)])
@pytest.mark.parametrize("kind", KINDS)
def test_plan_invariants_long_codes(kind, N, K, harness):
    """R1 nodes above 32 elements (the R1 slab scratch, r1_large), many depths in the slab."""
    from quantized_decoder_polar_codes_amd import lut as LU

    p = LU.random_luts(N, 16, seed=3 * N + K, distinct_mags=3)
    sweep(harness, kind, N, K, p, list_sizes(kind), SWEEP)


@pytest.fixture(scope="module")
def long_tables():
    """Tie-heavy random tables per N, made once for the four kinds."""
    from quantized_decoder_polar_codes_amd import lut as LU

    made = {}

    def get(N):
        if N not in made:
            made[N] = LU.random_luts(N, 16, seed=3 * N + 1, distinct_mags=3)
        return made[N]

    return get


# default, the smallest and the largest LDS budget (the whole tree in the slab / every depth the budget
# admits in LDS), and the switches that change which fields and rows a record packs
LONG_SWEEP = [{}, {"lds_budget": 256}, {"lds_budget": 65536}, {"no_pw1": True}, {"no_bc2": True}, {"no_trim": True},
              {"no_pfx": True}]


@pytest.mark.parametrize("N", [8192, 16384, 65536])
@pytest.mark.parametrize("kind", KINDS)
def test_plan_invariants_very_long_codes(kind, N, harness, long_tables):
    """The four deepest trees qpd_create accepts (n = 13, 14, 16; 4096 and 32768 differ from their neighbours
    in no field width) at a low, a half and a high rate: row numbers beside the 16 bits MF_BC2 packs them
    into, pointer fields at the last nibbles of the word (the leaf level of n = 16 takes nibble 0: u_field),
    R1 nodes of thousands of elements.  The only refusal is the W16 one (sweep asserts it).

    Measured on one core, N = 8192 / 16384 / 65536: random_luts 0.1 / 0.5 / 0.9 s, the BEC construction and
    identify_nodes below 0.02 s, from_packed(create=False) 1 ms, ph_check 0.03 / 0.05 / 0.15 s per switch
    setting; the whole test (12 cases) 29 s, its slowest case (SCL-LUT, N = 65536) 8 s."""
    p = long_tables(N)
    for K in rates(N):
        fm, nt = code(N, K)
        big = max(r1_sizes(nt, N))
        if K == 3 * N // 4:
            assert big >= N // 4  # R1 nodes far above 32 elements (r1_large, the slab's H / K / I rows)
        r = sweep(harness, kind, N, K, p, [8, 16] if "SCL" in kind else [1], LONG_SWEEP)
        assert r is not None
        if kind == "FastSCL-LUT" and big > 32:  # L = 16 is refused under every setting, L = 8 planned
            assert r[0] == {(16, tuple(kw.items())) for kw in LONG_SWEEP}
        else:
            assert not r[0]


def test_packed_fields_round_trip(harness):
    """check_packed of the harness notices a row that does not fit the 16 bits above MF_BC2's pointer
    fields: a copy of a planned record with row 40000 packed into it reads back negative."""
    from quantized_decoder_polar_codes_amd import decoders as D
    from quantized_decoder_polar_codes_amd import lut as LU

    N, K = 1024, 512
    fm, nt = code(N, K)
    dec = D.from_packed("SCL-LUT", LU.random_luts(N, 16, seed=7, distinct_mags=3), K, fm, L=8, create=False)
    harness.ph_pack_selftest.argtypes = [ctypes.c_void_p, ctypes.POINTER(Switches), ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    harness.ph_pack_selftest.restype = ctypes.c_int

    def selftest(row, **kw):
        msg = ctypes.create_string_buffer(256)
        sw = switches(**kw)
        return harness.ph_pack_selftest(ctypes.byref(dec._cfg), ctypes.byref(sw), row, msg, len(msg)), msg.value.decode()

    for kw in ({}, {"no_pw1": True}):
        assert selftest(0, **kw) == (0, "") and selftest(123, **kw) == (0, "") and selftest(32767, **kw) == (0, "")
        assert selftest(40000, **kw) == (1, "pad1 >> 16 gives row -25536, the plan packed row 40000")
        assert selftest(32768, **kw)[0] == 1
    assert selftest(0, no_bc2=True)[0] == -1  # no MF_BC2 record to copy


@pytest.mark.parametrize("golden", ["sclut_n128_k32_mindist", "scllut_n1024_k512_l8_mindist", "fastscllut_n1024_k512_l8_mindist"])
@pytest.mark.parametrize("kind", KINDS)
def test_plan_invariants_mindistortion_tables(kind, golden, harness):
    """One quanta row per node: MF_VUNI, rank words in the op record, mixed bottom subtrees, folded special nodes."""
    p = golden_packed(load_golden(os.path.join(GOLDEN_DIR, golden + ".npz")))
    seen = 0
    for K in rates(p.N):
        r = sweep(harness, kind, p.N, K, p, list_sizes(kind), SWEEP)
        if r is not None:
            seen |= r[1]
    if kind.startswith("Fast"):
        assert seen & MF_VUNI
    if kind == "FastSCL-LUT":
        assert seen & MF_BOTX and seen & MF_R1_RK and seen & MF_SFG


def test_plan_refusals_are_stated(harness):
    """The W16 FastSCL-LUT plan refuses an R1 node it cannot serve, with qpd_create's code and message: the
    64-element R1 node of (512, 256) at L = 12 and 16, under every switch setting; L <= 8 plans it (r1_large)."""
    from quantized_decoder_polar_codes_amd import lut as LU

    N, K = 512, 256
    fm, nt = code(N, K)
    assert max(r1_sizes(nt, N)) == 64
    refused, _ = sweep(harness, "FastSCL-LUT", N, K, LU.random_luts(N, 16, seed=5, distinct_mags=3), [8, 12, 16], SWEEP)
    assert refused == {(L, tuple(kw.items())) for L in (12, 16) for kw in SWEEP}
    refused, _ = sweep(harness, "SCL-LUT", N, K, LU.random_luts(N, 16, seed=5, distinct_mags=3), [8, 12, 16], SWEEP)
    assert not refused
