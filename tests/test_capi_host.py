"""The C-ABI's host-only logic checked on the CPU (g++, no HIP).

csrc/qpd_chunk.hpp: the per-decoder chunk buffer's policy -- grow on demand,
halve on an allocation failure, keep the smaller size.  No GPU test may reach
the fallback (an out-of-memory is not provoked on a device), so
tests/native/chunk_check.cpp runs it against a scripted allocator, as a
stand-alone program under AddressSanitizer and UBSan.

csrc/qpd_config.hpp: what qpd_create decides before it touches the device
(tests/native/config_harness.cpp through ctypes) -- every refusal of validate
with its message, the engine choice against the rule of DESIGN.md §1, the
generic engine's scratch rows against rows worked out by hand, the CRC taps.
"""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from quantized_decoder_polar_codes_amd import _lib as Q

CSRC = os.path.join(ROOT, "quantized_decoder_polar_codes_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")
E_INVALID, E_UNSUPPORTED = -1, -2
AUTO, GENERIC, FAST = 0, 1, 2
DOM_LUT, DOM_FLOAT = 0, 1
FAST_REFUSAL = ("fast engine needs LUT symbols with one table per node (f_step = g_step = 0), v <= 16 and L <= 8 "
                "(SCL-LUT and, on request, FastSCL-LUT: L <= 16)")


def compile_native(name, out, flags, headers):
    """tests/native/<name> built into tests/_build/<out> when it or a header it includes is newer."""
    os.makedirs(BUILD, exist_ok=True)
    dst = os.path.join(BUILD, out)
    src = os.path.join(ROOT, "tests", "native", name)
    deps = [src] + [os.path.join(CSRC, h) for h in headers]
    if not os.path.exists(dst) or any(os.path.getmtime(d) > os.path.getmtime(dst) for d in deps):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC, src]
                       + flags + ["-o", dst + ".tmp"], check=True)
        os.replace(dst + ".tmp", dst)
    return dst


def test_chunk_buffer_policy():
    exe = compile_native("chunk_check.cpp", "chunk_check", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                         ["qpd_chunk.hpp"])
    # the program counts its own live blocks; the leak checker needs ptrace, which a sandbox may deny
    r = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


@pytest.fixture(scope="module")
def harness():
    so = compile_native("config_harness.cpp", "config_harness.so", ["-fPIC", "-shared"],
                        ["qpd_config.hpp", "qpd_schedule.hpp", "qpd_types.hpp", "stl_sort.hpp"])
    L = ctypes.CDLL(so)
    L.ch_validate.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p]
    L.ch_engine.argtypes = [ctypes.c_int] * 7 + [ctypes.c_char_p, ctypes.c_int]
    L.ch_layout.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p]
    L.ch_layout.restype = None
    L.ch_crc_taps.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    L.ch_crc_taps.restype = ctypes.c_uint32
    L.ch_host_max_frames.argtypes = [ctypes.c_int] * 3
    L.ch_host_max_frames.restype = ctypes.c_int64
    return L


# ---- validate ---------------------------------------------------------------------------------------------------

N, K, V = 8, 4, 4


def config(kind, **spoil):
    """The smallest valid configuration of `kind` (N = 8, K = 4, v = 4, one table for every node), then
    `spoil`: fields set to another value, or (array name, index, value) entries under "poke".  Returns
    (QpdConfig, the arrays it points to)."""
    a = {
        "frozen_bits": np.array([1, 1, 1, 0, 1, 0, 0, 0], dtype=np.int32),
        "node_type": np.full(2 * N - 1, -1, dtype=np.int32),
        "lut_f": np.zeros(V * V, dtype=np.uint8), "f_base": np.zeros(N - 1, dtype=np.int32),
        "lut_g": np.zeros(2 * V * V, dtype=np.uint8), "g_base": np.zeros(N - 1, dtype=np.int32),
        "vcl": np.zeros(3 * N * V, dtype=np.float64),
        "crc_loc": np.array([0, 1, 2], dtype=np.int32),
        "r_f": np.ones(N - 1), "r_g": np.ones(N - 1),
        "q_bnd": np.zeros(3), "q_rec": np.zeros(4),
        "bnd_off": np.zeros(2 * (N - 1), dtype=np.int32), "bnd_len": np.full(2 * (N - 1), 3, dtype=np.int32),
        "rec_off": np.zeros(2 * (N - 1), dtype=np.int32), "rec_len": np.full(2 * (N - 1), 4, dtype=np.int32),
    }
    for name, i, val in spoil.pop("poke", ()):
        a[name][i] = val
    f = dict(kind=kind, N=N, K=K, L=4, v=V, lut_f_count=1, f_step=0, lut_g_count=1, g_step=0, vcl_rows=3, device=-1,
             max_waves=0, engine=AUTO, A=2, crc_n=2, crc_loc_count=3, q_bnd_count=3, q_rec_count=4)
    f.update({k: a[k].ctypes.data for k in a})
    f.update(spoil)
    return Q.QpdConfig(**f), a


def validate(harness, cfg):
    msg = ctypes.create_string_buffer(256)
    out = np.full(3, -9, dtype=np.int32)
    rc = harness.ch_validate(ctypes.byref(cfg) if cfg is not None else None, msg, len(msg), out.ctypes.data)
    return rc, msg.value.decode(), out.tolist()


@pytest.mark.parametrize("kind, n_fam_dom", [
    (Q.QPD_SC_LUT, [3, Q.QPD_SC_LUT, 0]), (Q.QPD_FASTSCL_LUT, [3, Q.QPD_FASTSCL_LUT, 0]),
    (Q.QPD_CASCL_LUT, [3, Q.QPD_SCL_LUT, 0]), (Q.QPD_CAFASTSCL_LUT, [3, Q.QPD_FASTSCL_LUT, 0]),
    (Q.QPD_CASCL_FLOAT, [3, Q.QPD_SCL_LUT, 1]), (Q.QPD_FASTSC_FLOAT, [3, Q.QPD_FASTSC_LUT, 1]),
    (Q.QPD_SCL_UNIFORM, [3, Q.QPD_SCL_LUT, 2]), (Q.QPD_SC_LLOYD, [3, Q.QPD_SC_LUT, 3])])
def test_validate_accepts_the_base_config(harness, kind, n_fam_dom):
    cfg, keep = config(kind)
    assert validate(harness, cfg) == (0, "", n_fam_dom)


# (kind, what is spoiled, code, message): one case per refusal of validate
REFUSALS = [
    (99, {}, E_INVALID, "unknown decoder kind"),
    (Q.QPD_CASCL_LUT, {"crc_n": 0}, E_INVALID, "crc_n must be in [1, 32]"),
    (Q.QPD_CASCL_LUT, {"crc_n": 33}, E_INVALID, "crc_n must be in [1, 32]"),
    (Q.QPD_CASCL_FLOAT, {"A": 3}, E_INVALID, "CASCLDecoder needs 1 <= A and A + crc_n <= K"),
    (Q.QPD_CASCL_FLOAT, {"A": 0}, E_INVALID, "CASCLDecoder needs 1 <= A and A + crc_n <= K"),
    (Q.QPD_CASCL_LUT, {"A": 1}, E_INVALID, "CRC-aided kinds need 1 <= A <= K and K - A <= crc_n"),  # K - A = 3 > crc_n
    (Q.QPD_CAFASTSCL_LUT, {"A": 5}, E_INVALID, "CRC-aided kinds need 1 <= A <= K and K - A <= crc_n"),
    (Q.QPD_CASCL_LUT, {"crc_loc": None}, E_INVALID, "bad crc_loc"),
    (Q.QPD_CASCL_LUT, {"crc_loc_count": -1}, E_INVALID, "bad crc_loc"),
    (Q.QPD_CASCL_LUT, {"poke": [("crc_loc", 2, 3)]}, E_INVALID, "crc_loc entry outside [0, crc_n]"),
    (Q.QPD_SC_LUT, {"N": 12}, E_INVALID, "N must be a power of two in [2, 65536]"),
    (Q.QPD_SC_LUT, {"N": 1}, E_INVALID, "N must be a power of two in [2, 65536]"),
    (Q.QPD_SC_LUT, {"N": 1 << 17}, E_INVALID, "N must be a power of two in [2, 65536]"),
    (Q.QPD_SC_LUT, {"frozen_bits": None}, E_INVALID, "frozen_bits is NULL"),
    (Q.QPD_SC_LUT, {"poke": [("frozen_bits", 0, 2)]}, E_INVALID, "frozen_bits entries must be 0 or 1"),
    (Q.QPD_SC_LUT, {"K": 5}, E_INVALID, "K must equal the number of information (0) entries of frozen_bits"),
    (Q.QPD_SCL_LUT, {"L": 33}, E_UNSUPPORTED, "list size L must be in [1, 32]"),
    (Q.QPD_SCL_FLOAT, {"L": 0}, E_UNSUPPORTED, "list size L must be in [1, 32]"),
    (Q.QPD_FASTSC_LUT, {"node_type": None}, E_INVALID, "node_type is required for the Fast decoders"),
    (Q.QPD_FASTSC_LUT, {"poke": [("node_type", 0, 3)]}, E_UNSUPPORTED,
     "root node labelled special (undefined behaviour in the reference)"),
    (Q.QPD_FASTSCL_FLOAT, {"poke": [("node_type", 0, 0)]}, E_UNSUPPORTED,
     "root node labelled special (undefined behaviour in the reference)"),
    (Q.QPD_SC_UNIFORM, {"r_g": None}, E_INVALID, "uniform kinds need r_f and r_g"),
    (Q.QPD_SC_LLOYD, {"rec_len": None}, E_INVALID, "Lloyd kinds need boundary and reconstruction tables"),
    # the last g table's list starts at 1 with 3 entries: one past q_bnd's 3
    (Q.QPD_SCL_LLOYD, {"poke": [("bnd_off", 2 * (N - 1) - 1, 1)]}, E_INVALID, "Lloyd boundary list outside q_bnd (or empty)"),
    (Q.QPD_SC_LLOYD, {"poke": [("bnd_len", 0, 0)]}, E_INVALID, "Lloyd boundary list outside q_bnd (or empty)"),
    (Q.QPD_SC_LLOYD, {"poke": [("rec_off", 3, -1)]}, E_INVALID, "Lloyd reconstruction list outside q_rec (or empty)"),
    (Q.QPD_SC_LLOYD, {"q_rec_count": 3}, E_INVALID, "Lloyd reconstruction list outside q_rec (or empty)"),
    (Q.QPD_SC_LUT, {"v": 257}, E_INVALID, "alphabet size v must be in [2, 256]"),
    (Q.QPD_SC_LUT, {"v": 1}, E_INVALID, "alphabet size v must be in [2, 256]"),
    (Q.QPD_SC_LUT, {"g_base": None}, E_INVALID, "null table pointer"),
    (Q.QPD_SC_LUT, {"f_step": 2}, E_INVALID, "f_step/g_step must be 0 or 1"),
    (Q.QPD_SC_LUT, {"vcl_rows": 2}, E_INVALID, "vcl_rows must be >= log2(N)"),
    (Q.QPD_SC_LUT, {"f_step": 1}, E_INVALID, "f_base/f_step index outside lut_f"),  # the root's 4 tables, 1 present
    (Q.QPD_SC_LUT, {"poke": [("f_base", 6, -1)]}, E_INVALID, "f_base/f_step index outside lut_f"),
    (Q.QPD_SC_LUT, {"poke": [("g_base", 6, 1)]}, E_INVALID, "g_base/g_step index outside lut_g"),
    (Q.QPD_SC_LUT, {"poke": [("lut_f", V * V - 1, V)]}, E_INVALID, "lut_f entry outside [0, v)"),
    (Q.QPD_SC_LUT, {"poke": [("lut_g", 2 * V * V - 1, V)]}, E_INVALID, "lut_g entry outside [0, v)"),
    (Q.QPD_SC_LUT, {"poke": [("vcl", 3 * N * V - 1, np.inf)]}, E_INVALID, "vcl rows 0..n-1 must be finite"),
]


def test_validate_null_config(harness):
    rc, msg, _ = validate(harness, None)
    assert (rc, msg) == (E_INVALID, "null config")


@pytest.mark.parametrize("kind, spoil, code, message", REFUSALS,
                         ids=[f"{i}-{m[:24].strip().replace(' ', '_')}" for i, (_, _, _, m) in enumerate(REFUSALS)])
def test_validate_refuses(harness, kind, spoil, code, message):
    cfg, keep = config(kind, **dict(spoil))
    rc, msg, _ = validate(harness, cfg)
    assert (rc, msg) == (code, message)


def test_refusal_list_covers_validate():
    """Every message validate can give has a case above."""
    import re

    with open(os.path.join(CSRC, "qpd_config.hpp")) as f:
        body = f.read().split("inline int validate(")[1].split("\ninline int choose_engine(")[0]
    said = set(re.findall(r'refuse\(err, QPD_E_\w+,\s*"([^"]+)"\)', body))
    assert len(said) >= 27
    assert said - {"null config"} == {m for _, _, _, m in REFUSALS}


# ---- engine choice ------------------------------------------------------------------------------------------------

def engine_rule(dom, f_step, v, kind, L, want):
    """the fast engine serves LUT symbols with one table per node and v <= 16, at L <= 8; at
    9 <= L <= 16 SCL-LUT under AUTO too and FastSCL-LUT only on request; everything else is the generic engine's,
    and asking for the fast engine there is refused."""
    serves = dom == DOM_LUT and f_step == 0 and v <= 16
    by_default = serves and (L <= 8 or (kind == Q.QPD_SCL_LUT and L <= 16))
    on_request = serves and kind == Q.QPD_FASTSCL_LUT and 9 <= L <= 16
    if want == FAST:
        return FAST if by_default or on_request else E_UNSUPPORTED
    return FAST if want == AUTO and by_default else GENERIC


def engine(harness, dom, f_step, g_step, v, kind, L, want):
    msg = ctypes.create_string_buffer(256)
    e = harness.ch_engine(dom, f_step, g_step, v, kind, L, want, msg, len(msg))
    return e, msg.value.decode()


def test_engine_choice_grid(harness):
    kinds = (Q.QPD_SC_LUT, Q.QPD_SCL_LUT, Q.QPD_FASTSC_LUT, Q.QPD_FASTSCL_LUT)
    for dom, f_step, v, kind, L, want in itertools.product((DOM_LUT, DOM_FLOAT), (0, 1), (16, 17), kinds,
                                                           (1, 8, 9, 16, 17, 32), (AUTO, GENERIC, FAST)):
        e, msg = engine(harness, dom, f_step, 0, v, kind, L, want)
        rule = engine_rule(dom, f_step, v, kind, L, want)
        assert (e, msg) == (rule, FAST_REFUSAL if rule == E_UNSUPPORTED else ""), (dom, f_step, v, kind, L, want)


def test_engine_choice_named_cases(harness):
    lut = (DOM_LUT, 0, 0, 16)
    assert engine(harness, *lut, Q.QPD_SCL_LUT, 16, AUTO) == (FAST, "")
    assert engine(harness, *lut, Q.QPD_SCL_LUT, 17, AUTO) == (GENERIC, "")
    for L in (9, 16):
        assert engine(harness, *lut, Q.QPD_FASTSCL_LUT, L, AUTO) == (GENERIC, "")
        assert engine(harness, *lut, Q.QPD_FASTSCL_LUT, L, FAST) == (FAST, "")
    assert engine(harness, *lut, Q.QPD_FASTSCL_LUT, 8, AUTO) == (FAST, "")
    assert engine(harness, *lut, Q.QPD_FASTSCL_LUT, 17, FAST) == (E_UNSUPPORTED, FAST_REFUSAL)
    assert engine(harness, *lut, Q.QPD_SC_LUT, 1, GENERIC) == (GENERIC, "")
    assert engine(harness, DOM_LUT, 0, 1, 16, Q.QPD_SC_LUT, 1, AUTO) == (GENERIC, "")  # per-element g tables
    assert engine(harness, DOM_LUT, 0, 1, 16, Q.QPD_SC_LUT, 1, FAST) == (E_UNSUPPORTED, FAST_REFUSAL)
    assert engine(harness, *lut, Q.QPD_SCL_LUT, 8, 7) == (FAST, "")  # QPD_ENGINE=7: not an engine id, AUTO


# ---- the generic engine's scratch rows ----------------------------------------------------------------------------

def layout(harness, kind, dom, n, max_r1):
    out = np.full(39, -9, dtype=np.int32)
    harness.ch_layout(kind, dom, 1 << n, n, max_r1, out.ctypes.data)
    return dict(So=out[:17].tolist(), Uo=out[17:34].tolist(), Ro=int(out[34]), Ho=int(out[35]), Ko=int(out[36]),
                Io=int(out[37]), rows=int(out[38]))


def padded(rows):
    return rows + [0] * (17 - len(rows))


def test_generic_layout_sc_lut_n8(harness):
    """A row is one dword per lane: 4 LUT symbols (bytes) or 32 partial-sum bits.  Depth 1 holds 4 symbols, depth
    2 holds 2: one row each.  The partial sums of depths 1..3 (4, 2, 1 bits) and the right chain (8 bits): one each."""
    g = layout(harness, Q.QPD_SC_LUT, DOM_LUT, 3, 0)
    assert g == dict(So=padded([0, 0, 1]), Uo=padded([0, 2, 3, 4]), Ro=5, Ho=6, Ko=6, Io=6, rows=6)


def test_generic_layout_float_n8(harness):
    """An fp64 value is two dword rows per element: depth 1 takes 2 * 4 rows, depth 2 takes 2 * 2."""
    g = layout(harness, Q.QPD_SCL_LUT, DOM_FLOAT, 3, 0)
    assert g == dict(So=padded([0, 0, 8]), Uo=padded([0, 12, 13, 14]), Ro=15, Ho=16, Ko=16, Io=16, rows=16)


@pytest.mark.parametrize("max_r1, want", [
    # N = 64: symbols of depths 1..5 = 32, 16, 8, 4, 2 -> 8, 4, 2, 1, 1 rows (0..15); partial sums of depths 1..6
    # one row each (16..21); the right chain's 64 bits two rows (22, 23).  Then the R1 node's hard decisions
    # (max_r1 bits: one row), its fp64 keys (2 * max_r1 rows) and its argsort indices, which take max_r1 rows of
    # their own only above libstdc++'s insertion-sort threshold of 16.
    (16, dict(Ho=24, Ko=25, Io=57, rows=57)),
    (32, dict(Ho=24, Ko=25, Io=89, rows=121)),
    (0, dict(Ho=24, Ko=24, Io=24, rows=24)),
])
def test_generic_layout_fastscl_r1_rows(harness, max_r1, want):
    g = layout(harness, Q.QPD_FASTSCL_LUT, DOM_LUT, 6, max_r1)
    assert g == dict(So=padded([0, 0, 8, 12, 14, 15]), Uo=padded([0, 16, 17, 18, 19, 20, 21]), Ro=22, **want)
    if max_r1:  # the R1 rows are FastSCL's alone
        assert layout(harness, Q.QPD_SCL_LUT, DOM_LUT, 6, max_r1)["rows"] == 24


# ---- the CRC tap word and the host engine's crossover ----------------------------------------------------------------

def test_crc_taps(harness):
    """Coefficient j of the generator is register bit crc_n - j; the leading coefficient (j = 0) drops out."""
    loc = np.array([0, 2, 7, 8], dtype=np.int32)
    assert harness.ch_crc_taps(8, loc.ctypes.data, 4) == (1 << 6) | (1 << 1) | 1
    assert harness.ch_crc_taps(8, None, 0) == 0
    loc32 = np.array([0, 1, 32], dtype=np.int32)
    assert harness.ch_crc_taps(32, loc32.ctypes.data, 3) == (1 << 31) | 1


def test_host_crossover_model(harness):
    """host_max_frames = GPU call cost / host cost per frame (csrc/qpd_config.hpp), at least one frame."""
    def model(N, n, L):
        nn = N * n
        host = 0.00136 * nn * L + (0.005 * L * N if L > 1 else 0.0) + 1.6
        gpu = 55.0 + 0.083 * nn + (0.02 * nn if L > 1 else 0.0)
        return max(1, int(gpu / host))

    for N, n, L in ((8, 3, 1), (128, 7, 1), (1024, 10, 1), (1024, 10, 8), (65536, 16, 32)):
        assert harness.ch_host_max_frames(N, n, L) == model(N, n, L)
    assert harness.ch_host_max_frames(65536, 16, 32) == 1
