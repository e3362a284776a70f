"""Rows in lookup order (QPD_ROW_BYTEIDX, csrc/qpd_fast_switches.hpp), checked on the plan (CPU).

The plan compiler (csrc/qpd_plan.hpp, built with g++ by tests/native/plan_row_order_harness.cpp) marks the ops of
the plain kinds' plans MF_LO: every S row of M >= 8 symbols holds element 4w + j in the high nibble of byte j of
word w and element 4w + j + M/2 in the low one.  This test walks the op lists -- the prefix stages', then the
decode kernel's -- with a symbolic model of the rows in which every nibble carries (node, element), each op moving
nibbles exactly as its kernel code does (fg_op, ff_op, gsel_op, fg_chan_op, bot3_op, the pre-pass kernels, the
prefix stages' exports and imports; csrc/qpd_fast_lookup.hpp, qpd_fast_bot.hpp, qpd_fast_pre.hpp), and asserts

  * every f / g op's index byte k is (element e, element e + M/2) of the op's own node, as it lies;
  * every word an f / g op stores is the child row's word in lookup order;
  * every BOT3 receives W3 in its interleaved order (the folded ones their parent's 16 symbols as two index words);
  * FastSC-LUT / FastSCL-LUT plans carry no MF_LO and are byte for byte those of a build with the switch off, and
    the plain kinds' plans differ from that build's in the MF_LO bit alone.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from test_plan import BUILD, CSRC, Switches, code, switches
from conftest import ROOT

OP_F, OP_G, OP_BOT3, OP_IMPORT, OP_EXPORT = 0, 1, 9, 10, 11
MF_SRC_LDS, MF_DST_LDS, MF_CHAN, MF_PRE, MF_GSEL, MF_BFG, MF_BG = 1, 2, 64, 256, 512, 1024, 2048
MF_ZERO, MF_PM, MF_XBUF, MF_FF, MF_FF_DL, MF_LO = 16384, 32768, 262144, 524288, 1048576, 1 << 30
FIELDS = ("type", "flags", "d", "node", "cnt", "src_row", "dst_row", "u_row", "r_row", "sh_src", "sh_u", "sh_dst", "tab",
          "vrow", "tab2", "pad1")
STAGE_BUFFER = {0: 1, 1: 3, 2: 2}  # the record buffer a prefix list exports to (OP_IMPORT's `node`)


def _load(name, extra):
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, name)
    src = os.path.join(ROOT, "tests", "native", "plan_row_order_harness.cpp")
    deps = [src] + [os.path.join(CSRC, f) for f in ("qpd_plan.hpp", "qpd_mop.hpp", "qpd_schedule.hpp", "qpd_types.hpp",
                                                    "qpd_fast_switches.hpp", "stl_sort.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-I", os.path.join(ROOT, "include"), "-I", CSRC]
                       + extra + [src, "-o", so + ".tmp"], check=True)
        os.replace(so + ".tmp", so)
    L = ctypes.CDLL(so)
    L.pro_plan.argtypes = [ctypes.c_void_p, ctypes.POINTER(Switches), ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.pro_plan.restype = ctypes.c_int
    assert L.pro_switches_size() == ctypes.sizeof(Switches)
    return L


@pytest.fixture(scope="module")
def product():
    return _load("plan_row_order.so", [])


@pytest.fixture(scope="module")
def switched_off():
    L = _load("plan_row_order_off.so", ["-DQPD_ROW_BYTEIDX=0"])
    assert L.pro_row_byteidx() == 0
    return L


_TABLES = {}


def plan(harness, kind, N, K, L, **sw):
    """(lists of op dicts [stage 1, stage 1b, stage 2, decode], info, the raw records) or None if refused."""
    from quantized_decoder_polar_codes_amd import decoders as D
    from quantized_decoder_polar_codes_amd import lut as LU

    if N not in _TABLES:
        _TABLES[N] = LU.random_luts(N, 16, seed=N, distinct_mags=3)
    fm, nt = code(N, K)
    if kind.startswith("Fast") and 0 <= nt[0] <= (3 if kind == "FastSC-LUT" else 2):
        return None
    dec = D.from_packed(kind, _TABLES[N], K, fm, L=L, node_type=nt, create=False)
    cap = 16 * N
    raw = np.zeros((cap, 16), dtype=np.int32)
    counts, info = np.zeros(4, dtype=np.int32), np.zeros(4, dtype=np.int32)
    s = switches(**sw)
    n = harness.pro_plan(ctypes.byref(dec._cfg), ctypes.byref(s), raw.ctypes.data, cap, counts.ctypes.data, info.ctypes.data)
    if n == -2:
        return None
    assert n >= 0, n
    raw = raw[:n].copy()
    lists, at = [], 0
    for c in counts:
        lists.append([dict(zip(FIELDS, (int(x) for x in r))) for r in raw[at:at + c]])
        at += c
    return lists, dict(zip(("row_lo", "pre", "sets", "lds_from"), (int(x) for x in info))), (raw, counts.copy())


def lo_word(node, M, w):
    """Word w of the row of node's M symbols in lookup order: nibble i -> (node, element)."""
    out = [None] * 8
    for j in range(4):
        out[2 * j + 1] = (node, 4 * w + j)
        out[2 * j] = (node, 4 * w + j + M // 2)
    return out


def il_nib(k):  # il_nib<8> (qpd_fast_lookup.hpp)
    return 2 * k + 1 if k < 4 else 2 * (k - 4)


class Rows:
    """The symbolic state: slab / LDS rows, the frame's pre-pass row, the prefix stages' records."""

    def __init__(self, N, pre):
        self.N, self.mem, self.rec = N, {}, {}
        self.pre = {}
        if pre:  # root_pre_kernel<In, true>: [f(y) | g(y, 0) | g(y, 1)], N/16 words each, S[1] in lookup order
            nw = N // 16
            for w in range(nw):
                self.pre[w] = lo_word((1, 0), N // 2, w)
                self.pre[nw + w] = self.pre[2 * nw + w] = lo_word((1, 1), N // 2, w)

    def ld(self, lds, row, what):
        word = self.mem.get((bool(lds), row))
        assert word is not None, f"{what}: reads row {row} ({'LDS' if lds else 'slab'}) that holds no symbols"
        return word

    def st(self, lds, row, word):
        self.mem[(bool(lds), row)] = word


def index_bytes(word, node, M, what):
    """The four index bytes of a stored word as lut_lds / lut_vec (LO) take them: byte k = (high nibble, low
    nibble) must be (element e, element e + M/2) of `node`.  Returns the four e."""
    out = []
    for k in range(4):
        hi, lo = word[2 * k + 1], word[2 * k]
        assert hi is not None and lo is not None, f"{what}: byte {k} holds no symbols"
        assert hi[0] == node and lo[0] == node, f"{what}: byte {k} holds {hi}, {lo}, not symbols of node {node}"
        assert lo[1] == hi[1] + M // 2 and hi[1] < M // 2, f"{what}: byte {k} pairs elements {hi[1]} and {lo[1]} of {M}"
        out.append(hi[1])
    return out


def lookup_word(A, B, node, M, child, what):
    """lut_lds / lut_vec <8, IL, LO>: A's bytes give the high nibbles, B's the low ones."""
    ea, eb = index_bytes(A, node, M, what + " (a)"), index_bytes(B, node, M, what + " (b)")
    out = [None] * 8
    for k in range(4):
        out[2 * k + 1] = (child, ea[k])
        out[2 * k] = (child, eb[k])
    return out


def walk(lists, info, N, label):
    """Runs the lists on the symbolic rows; returns what was checked: (f/g words, BOT3s)."""
    n = N.bit_length() - 1
    R = Rows(N, info["pre"])
    words = bots = 0
    for li, ops in enumerate(lists):
        for i, m in enumerate(ops):
            fl, what = m["flags"], f"{label} list {li} op {i} (type {m['type']}, d {m['d']}, node {m['node']}, flags {m['flags']:#x})"
            if m["type"] == OP_EXPORT:
                for w in range(m["cnt"]):
                    R.rec[(STAGE_BUFFER[li], m["dst_row"] + w)] = R.mem.get((bool(fl & MF_SRC_LDS), m["src_row"] + w))
            elif m["type"] == OP_IMPORT:
                if (fl & MF_XBUF) and not (fl & MF_PM):
                    for w in range(m["cnt"]):
                        R.st(fl & MF_DST_LDS, m["dst_row"] + w, R.rec.get((m["node"], m["src_row"] + w)))
            elif m["type"] in (OP_F, OP_G):
                assert fl & MF_LO, what + ": no MF_LO"
                c = m["cnt"]
                if c < 8:
                    continue  # rows of < 8 symbols keep the element order (N < 16 only)
                node, child, M, nwo = (m["d"], m["node"]), (m["d"] + 1, 2 * m["node"] + (m["type"] == OP_G)), 2 * c, c >> 3
                out = []
                for w in range(nwo):
                    if fl & MF_GSEL:  # a nibble select between the two g rows: the word's order is theirs
                        g0, g1 = R.pre[m["src_row"] + w], R.pre[m["src_row"] + nwo + w]
                        assert g0 == g1, what
                        o = list(g0)
                    elif fl & MF_CHAN:  # fg_chan_op<.., LO>: four runs of four channel symbols, lut_vec<8, IL>
                        a = [4 * w + j for j in range(4)] + [4 * (nwo + w) + j for j in range(4)]
                        b = [4 * (2 * nwo + w) + j for j in range(4)] + [4 * (3 * nwo + w) + j for j in range(4)]
                        o = [None] * 8
                        for k in range(8):
                            assert b[k] == a[k] + M // 2, what
                            o[il_nib(k)] = (child, a[k])
                    else:
                        if fl & MF_PRE:
                            A, B = R.pre[m["src_row"] + w], R.pre[m["src_row"] + nwo + w]
                        else:
                            A = R.ld(fl & MF_SRC_LDS, m["src_row"] + w, what)
                            B = R.ld(fl & MF_SRC_LDS, m["src_row"] + nwo + w, what)
                        o = lookup_word(A, B, node, M, child, what + f" word {w}")
                    assert o == lo_word(child, c, w), f"{what}: stores word {w} as {o}"
                    R.st(fl & MF_DST_LDS, m["dst_row"] + w, o)
                    out.append(o)
                    words += 1
                if fl & MF_FF:  # ff_op: the left child's f from the words just computed
                    nwc, gc = nwo >> 1, (m["d"] + 2, 2 * child[1])
                    for u in range(nwc):
                        o = lookup_word(out[u], out[u + nwc], child, c, gc, what + f" child word {u}")
                        assert o == lo_word(gc, c // 2, u), f"{what}: stores child word {u} as {o}"
                        R.st(fl & MF_FF_DL, m["r_row"] + u, o)
                        words += 1
            elif m["type"] == OP_BOT3:
                assert fl & MF_LO, what + ": no MF_LO"
                assert m["d"] == n - 3
                node = (m["d"], m["node"])
                if fl & MF_BFG:
                    parent = (m["d"] - 1, m["node"] >> 1)
                    assert bool(fl & MF_BG) == bool(m["node"] & 1), what
                    a = R.ld(fl & MF_SRC_LDS, m["src_row"], what)
                    b = R.ld(fl & MF_SRC_LDS, m["src_row"] + 1, what)
                    w3 = lookup_word(a, b, parent, 16, node, what)
                elif fl & MF_CHAN:
                    bots += 1
                    continue  # N = 8: the channel's word is permuted once (nib_interleave8)
                elif fl & MF_PRE:
                    w3 = R.pre[m["src_row"]]
                else:
                    w3 = R.ld(fl & MF_SRC_LDS, m["src_row"], what)
                assert w3 == lo_word(node, 8, 0), f"{what}: W3 arrives as {w3}"
                bots += 1
    return words, bots


SWEEP = [{}, {"sets": 1}, {"no_pre": True}, {"no_pfx": True}, {"no_pfx2": True}, {"pfx1b": True}, {"no_bfuse": True},
         {"no_ff": True}, {"no_bc2": True}, {"no_pw1": True}, {"no_trim": True}, {"lds_budget": 2048}, {"lds_budget": 65536}]


@pytest.mark.parametrize("N", [16, 32, 64, 1024])
@pytest.mark.parametrize("kind,L", [("SC-LUT", 1), ("SCL-LUT", 8), ("SCL-LUT", 16), ("SCL-LUT", 4)])
def test_rows_in_lookup_order(kind, L, N, product):
    assert product.pro_row_byteidx() == 1, "the product is built with QPD_ROW_BYTEIDX on"
    seen_words = seen_bots = 0
    for K in sorted({N // 2, max(1, N // 4), 3 * N // 4, N}):
        for sw in SWEEP:
            got = plan(product, kind, N, K, L, **sw)
            assert got is not None
            lists, info, _ = got
            assert info["row_lo"] == 1
            w, b = walk(lists, info, N, f"{kind} L={L} N={N} K={K} {sw}")
            seen_words += w
            seen_bots += b
    assert seen_bots > 0 and (seen_words > 0 or N < 32)


@pytest.mark.parametrize("N", [16, 32, 64, 1024])
@pytest.mark.parametrize("kind,L", [("FastSCL-LUT", 8), ("FastSCL-LUT", 16), ("FastSC-LUT", 1), ("SCL-LUT", 8), ("SC-LUT", 1)])
def test_switch_changes_the_flag_alone(kind, L, N, product, switched_off):
    """Fast kinds: the plans are byte for byte those of the build with the switch off; plain kinds: but for MF_LO."""
    planned = 0
    for K in sorted({N // 2, max(1, N // 4), 3 * N // 4}):
        for sw in SWEEP:
            a, b = plan(product, kind, N, K, L, **sw), plan(switched_off, kind, N, K, L, **sw)
            assert (a is None) == (b is None)
            if a is None:
                continue
            planned += 1
            (ra, ca), (rb, cb) = a[2], b[2]
            assert np.array_equal(ca, cb) and b[1]["row_lo"] == 0
            if kind.startswith("Fast"):
                assert a[1] == b[1] and np.array_equal(ra, rb), f"{kind} N={N} K={K} {sw}: the plan changed with the switch"
                assert not (ra[:, 1] & MF_LO).any()
            else:
                assert a[1]["row_lo"] == 1 and not (rb[:, 1] & MF_LO).any()
                masked = ra.copy()
                masked[:, 1] &= ~np.int32(MF_LO)
                assert np.array_equal(masked, rb), f"{kind} N={N} K={K} {sw}: more than MF_LO changed"
                fg = np.isin(ra[:, 0], (OP_F, OP_G, OP_BOT3))
                assert ((ra[:, 1] & MF_LO) != 0).tolist() == fg.tolist()
    assert planned > 0 or kind.startswith("Fast")
