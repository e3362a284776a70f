"""Cases, inputs and oracle references of the decode-status sweep: shared by
tests/test_oracle_status.py (CPU: the oracle's status against the host engine, the
planner's choice per case, the conditions that keep a comparison informative) and
tests/test_gpu_status_sweep.py (the kernels against the oracle).

A Case names one decoder (kind, code, list size, tables or re-quantizer, engine,
planner switches) and the frames it decodes.  reference(case) gives its inputs
and, per CRC mask, the oracle's (bits, pml, winner, passed), computed once per
process for all cases that differ only in engine or switches.  EXPECT holds, per
case id, the kernel instantiation the case is there to reach, as the planner
chose it when the case was written (test_oracle_status.py re-plans every case on
the CPU and compares; the GPU sweep compares with qpd_info).
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np

import code_masks as M

CRC24_LOC = (24, 23, 21, 20, 17, 15, 13, 12, 8, 4, 2, 1, 0)
CRC11_LOC = (11, 10, 9, 5, 0)
FAST, GENERIC = 2, 1  # qpd_info.engine
LUT_KINDS = ("SCL-LUT", "FastSCL-LUT", "CA-SCL-LUT", "CA-FastSCL-LUT")
FLOAT_KINDS = ("SCL", "FastSCL", "SCL-Uniform", "SCL-Lloyd", "CA-SCL")
SWITCH_ENV = ("QPD_NO_PFX", "QPD_NO_PRE", "QPD_PFX1B", "QPD_SETS", "QPD_LDS_BUDGET", "QPD_PRE_CHUNK", "QPD_U8_CHUNK",
              "QPD_NO_PW1", "QPD_ENGINE")


class Case(NamedTuple):
    kind: str
    N: int
    K: int
    L: int
    tables: str = "random"  # LUT: random / continuous / minsum / perelem; float: the float_inputs style
    engine: str = "auto"    # LUT: auto / fast / generic; float kinds have the generic kernel only
    env: tuple = ()         # planner switches, (name, value) pairs
    A: int = 0              # CRC-aided: message bits
    crc_n: int = 0
    ebn0: float = 0.0       # CRC-aided: the channel of the CRC-carrying frames
    B: int = 96
    v: int = 16
    mask: str = ""          # frozen mask of tests/code_masks.py instead of the reliability order's ("random<seed>")
    max_waves: int = 0
    dtype: str = "i32"      # LUT: i32 / u8 symbols
    seed: int = 0           # of the frames (and of random tables), beside what the code's sizes give
    unmet: str = ""         # conditions of check_informative this case cannot meet, by name; why is in UNMET

    @property
    def id(self):
        s = f"{self.kind}-{self.N}-{self.K}-{self.L}-{self.tables}-{self.engine}"
        if self.A:
            s += f"-A{self.A}c{self.crc_n}"
        for name, on in ((f"v{self.v}", self.v != 16), (self.mask, self.mask), (f"B{self.B}", self.B != 96),
                         (f"mw{self.max_waves}", self.max_waves), (self.dtype, self.dtype != "i32")):
            if on:
                s += "-" + name
        return s + "".join(f"-{k[4:]}{v}" for k, v in self.env)

    @property
    def is_float(self):
        return self.kind in FLOAT_KINDS

    @property
    def crc_loc(self):
        return CRC24_LOC if self.crc_n == 24 else CRC11_LOC

    @property
    def nchk(self):
        """Check bits compared after the A message bits (include/qpd.h: K - A for the LUT kinds, crc_n for CA-SCL)."""
        return 0 if not self.A else self.crc_n if self.is_float else self.K - self.A

    @property
    def mask_sizes(self):
        return sorted({0, 1, min(16, self.crc_n), self.crc_n}) if self.A else [0]

    def ref_key(self):
        """What the decoded result depends on: not the engine, its switches, the grid or the symbol type."""
        return self._replace(engine="", env=(), max_waves=0, dtype="i32", unmet="")


def crc_mask(bits):
    """The sweep's CRC mask of `bits` entries: seeded, its last entry 1 (a 1-bit mask flips the last check bit)."""
    m = np.random.default_rng(700 + bits).integers(0, 2, size=bits, dtype=np.uint8)
    if bits:
        m[-1] = 1
    return m


def code_of(case):
    """(frozen mask, node types, message positions) of the case's code."""
    from quantized_decoder_polar_codes_amd import codes as C

    if case.mask:
        fm = M.random_mask(case.N, case.K, int(case.mask[6:]))
        return fm, M.node_type_of(fm), np.flatnonzero(fm == 0)
    if case.N > 1024:  # beyond the 5G sequence: the BEC construction of tests/test_plan.py
        from test_plan import code

        fm, nt = code(case.N, case.K)
        return fm, nt, np.flatnonzero(fm == 0)
    _, mb, fm, _ = C.construct_pw(case.N, case.K)
    return fm, C.identify_nodes(case.N, mb).astype(np.int32), mb


def special_root(case):
    """FastSCL kinds on a code whose root is a special node: undefined in the reference, refused by the
    library and the oracle alike -- no such case is part of the sweep."""
    return "Fast" in case.kind and 0 <= code_of(case)[1][0] <= 2


def seed_of(case):
    return 9000 + case.N + 7 * case.L + 3 * case.K + case.v + 100003 * case.seed


@functools.lru_cache(maxsize=None)
def _tables(N, v, tables, seed):
    from quantized_decoder_polar_codes_amd import lut as LU

    if tables == "minsum":
        return LU.minsum_uniform_luts(N)
    if tables == "continuous":
        return LU.random_luts(N, v, seed=seed, distinct_mags=None)
    return LU.random_luts(N, v, seed=seed, distinct_mags=3, per_element=(tables == "perelem"))


def tables_of(case):
    return _tables(case.N, case.v, case.tables, seed_of(case))


def quant_of(case):
    from test_float_oracle import quant_for

    return quant_for(case.kind, case.N)


def crc_frames(case, rng):
    """BPSK + AWGN LLRs [B, N] of frames that carry the case's CRC, around the case's Eb/N0."""
    import oracle
    from quantized_decoder_polar_codes_amd import codes as C

    _, _, mb = code_of(case)
    msg = rng.integers(0, 2, size=(case.B, case.A), dtype=np.uint8)
    tail = np.zeros((case.B, case.K - case.A), dtype=np.uint8)
    chk = oracle.crc_encode(msg, case.crc_n, case.crc_loc)[:, : case.K - case.A]
    tail[:, : chk.shape[1]] = chk
    x = C.polar_encode(np.concatenate([msg, tail], axis=1), mb, case.N)
    # Eb/N0 spread over +-1.5 dB around the case's: long codes fail or pass almost together at one value, and
    # the comparison needs failing frames and frames the CRC decides in the same batch
    ebn0 = case.ebn0 + np.linspace(-1.5, 1.5, case.B)[:, None]
    sigma = np.sqrt(1 / (2 * (case.K / case.N) * 10 ** (ebn0 / 10)))
    return ((1.0 - 2.0 * x) + rng.normal(0, sigma, size=x.shape)) * 2 / sigma ** 2


def inputs_of(case):
    """The frames of a case: int32 symbols [B, N] (LUT kinds) or float64 LLRs."""
    from test_float_oracle import float_inputs

    rng = np.random.default_rng(seed_of(case))
    if case.is_float:
        if not case.A:
            return float_inputs(case.N, case.B, seed=seed_of(case), style=case.tables)
        llr = crc_frames(case, rng)  # the CRC must decide on some frames: codewords, in the style asked for
        return np.clip(np.rint(llr), -3, 3) if case.tables == "ties" else llr
    if case.A:
        return np.clip(np.rint(crc_frames(case, rng) / 0.5 + 7.5), 0, 15).astype(np.int32)
    x = rng.integers(0, case.v, size=(case.B, case.N), dtype=np.int32)
    if case.tables == "minsum":  # every other frame from the four weakest quanta: equal metrics at the end
        x[1::2] = rng.integers(6, 10, size=x[1::2].shape, dtype=np.int32)
    return x


@functools.lru_cache(maxsize=None)
def _reference(key):
    import oracle

    fm, nt, _ = code_of(key)
    x = inputs_of(key)
    out = {}
    for bits in key.mask_sizes:
        mask = crc_mask(bits) if bits else None
        if key.is_float:
            kw = dict(A=key.A, crc_n=key.crc_n, crc_loc=key.crc_loc, mask=mask) if key.A else {}
            out[bits] = oracle.decode_float_status(key.kind, key.N, key.K, fm, x, L=key.L, node_type=nt,
                                                   quant=quant_of(key), **kw)
        else:
            kw = dict(A=key.A, crc_n=key.crc_n, crc_loc=key.crc_loc, mask=mask) if key.A else {}
            out[bits] = oracle.decode_lut_status(key.kind, tables_of(key), key.K, key.L, fm, x, node_type=nt, **kw)
    return x, out


def reference(case):
    """(inputs, {mask bits: (bits, pml, winner, passed)}) of the oracle; shared, do not write to it."""
    return _reference(case.ref_key())


# Why a case cannot meet a condition of check_informative; the case names the conditions in Case.unmet, runs
# against the oracle all the same, and asserts every other condition.
UNMET = {
    # L = 2 on min-sum tables (channel values are odd multiples of half a quantum).  (4, 2, 2): of all 16^4 inputs
    # none ends with two equal metrics (tests/test_oracle_status.py decodes them all).  (32, 30, 2) with CRC:
    # no tie in any batch of the search (1536 frames at each of 15 Eb/N0, three seeds)
    "ties": "no input found, or none there is, that gives L = 2 equal final metrics on min-sum tables",
    # random tables decode nothing: no path of a frame carries a valid 24-bit CRC (chance 2^-24 per path), so
    # every frame fails, on the best-metric path, under every mask
    "late,mask": "random tables do not decode: no path passes the CRC, with or without a mask",
}


def informative_counts(case):
    """What check_informative counts, on the oracle's output alone: frames with a tie at the minimum metric,
    frames with any two equal final metrics, frames failing the CRC, frames passing on a path that is not
    rank 0, and per non-empty mask the frames whose winner or verdict it changes."""
    _, ref = reference(case)
    bits0, pml0, win0, pass0 = ref[0]
    ties = int(((pml0 == pml0.min(1, keepdims=True)).sum(1) > 1).sum())
    equal = int((np.diff(np.sort(pml0, axis=1), axis=1) == 0).any(1).sum())
    late = pass0 & (pml0[np.arange(len(win0)), win0] > pml0.min(1))  # passed above the best metric: not rank 0
    changed = {mb: int(((ref[mb][2] != win0) | (ref[mb][3] != pass0)).sum()) for mb in case.mask_sizes[1:]}
    return ties, equal, int((~pass0).sum()), int(late.sum()), changed


def check_informative(case):
    """The conditions under which an equal status says something, on the oracle's output alone."""
    _, ref = reference(case)
    ties, equal, fails, late, changed = informative_counts(case)
    unmet = set(case.unmet.split(",")) - {""}
    assert case.unmet in UNMET or not unmet, case.unmet
    # float kinds: the "ties" style is rounded LLRs, which tie on the plain SCL / FastSCL metric
    tie_heavy = case.tables in ("random", "minsum", "perelem") or (case.tables == "ties" and case.kind in ("SCL", "FastSCL"))
    if tie_heavy and "ties" not in unmet:
        assert ties >= 8, f"{case.id}: {ties} frames with a tie at the minimum metric"
    if case.tables == "continuous":
        assert equal == 0, f"{case.id}: equal final metrics on continuous tables"
    if not case.A:
        return
    assert fails >= 8, f"{case.id}: {fails} frames fail the CRC"
    if "late" not in unmet:
        assert late >= 8, f"{case.id}: {late} frames pass on a path that is not rank 0"
    for mb, n in changed.items():
        if case.crc_n - mb >= case.nchk:  # the mask lies wholly past the K - A compared bits: nothing may change
            assert n == 0 and (ref[mb][0] == ref[0][0]).all(), f"{case.id}: a mask on uncompared bits changed the result"
        elif "mask" in unmet:
            assert n == 0, f"{case.id}: {UNMET[case.unmet]}, yet the {mb}-bit mask changes {n} frames"
        else:
            assert n >= 8, f"{case.id}: the {mb}-bit mask changes {n} frames"


# ---------------------------------------------------------------------------------------------------------
# the sweep
# ---------------------------------------------------------------------------------------------------------

def _env(**kw):
    return tuple(sorted(kw.items()))


def _b(N):
    return 24 if N >= 1024 else 96  # check_informative counts to 8: no fewer than 16 frames anywhere but B = 1


# The frames of every CRC-aided decoder of the sweep: (kind, N, K, A, L, tables[, B]) -> (Eb/N0 in dB, the centre
# of the spread; seed; B).  Searched on the oracle alone -- Eb/N0 in steps of 0.5 dB, seeds 0..3, and B doubled
# from 96 (48 at N = 1024) only where no Eb/N0 and seed gave the counts of check_informative -- and kept here so
# that every run decodes the same frames.  An entry with B in its key is a launch seam, whose B is given.
CA_INPUTS = {
    ("CA-SCL-LUT", 128, 64, 40, 9, "minsum"): (-0.5, 0, 96),
    ("CA-SCL-LUT", 128, 64, 40, 16, "minsum"): (0.5, 0, 96),
    ("CA-SCL-LUT", 512, 256, 232, 9, "minsum"): (1.0, 0, 384),
    ("CA-SCL-LUT", 512, 256, 232, 16, "minsum"): (2.0, 0, 96),
    ("CA-FastSCL-LUT", 128, 64, 40, 9, "minsum"): (0.5, 1, 96),
    ("CA-FastSCL-LUT", 128, 64, 40, 12, "minsum"): (-0.5, 0, 96),
    ("CA-FastSCL-LUT", 128, 64, 40, 16, "minsum"): (0.5, 0, 96),
    ("CA-FastSCL-LUT", 512, 200, 176, 9, "minsum"): (2.0, 1, 768),
    ("CA-FastSCL-LUT", 512, 200, 176, 12, "minsum"): (2.0, 0, 384),
    ("CA-FastSCL-LUT", 512, 200, 176, 16, "minsum"): (0.5, 0, 768),
    ("CA-SCL-LUT", 256, 128, 104, 4, "minsum"): (0.5, 1, 96),
    ("CA-SCL-LUT", 64, 44, 20, 4, "minsum"): (0.5, 1, 96),
    ("CA-FastSCL-LUT", 64, 44, 20, 4, "minsum"): (0.0, 0, 192),
    ("CA-SCL-LUT", 128, 64, 40, 8, "minsum"): (0.0, 0, 96),
    ("CA-FastSCL-LUT", 128, 64, 40, 8, "minsum"): (0.0, 0, 96),
    ("CA-SCL-LUT", 128, 64, 40, 8, "random"): (-0.5, 0, 96),
    ("CA-FastSCL-LUT", 128, 64, 40, 8, "random"): (-0.5, 0, 96),
    ("CA-SCL-LUT", 128, 64, 40, 16, "random"): (-0.5, 0, 96),
    ("CA-FastSCL-LUT", 128, 64, 40, 16, "random"): (-0.5, 0, 96),
    ("CA-SCL-LUT", 256, 124, 100, 12, "minsum"): (2.0, 1, 96),
    ("CA-FastSCL-LUT", 256, 124, 100, 12, "minsum"): (2.0, 0, 192),
    ("CA-SCL-LUT", 256, 111, 100, 8, "minsum"): (1.0, 0, 192),
    ("CA-FastSCL-LUT", 256, 111, 100, 8, "minsum"): (0.0, 1, 96),
    ("CA-SCL-LUT", 512, 254, 230, 3, "minsum"): (1.0, 0, 384),
    ("CA-FastSCL-LUT", 512, 254, 230, 3, "minsum"): (1.5, 1, 384),
    ("CA-SCL", 64, 40, 29, 16, "awgn"): (-0.5, 0, 96),
    ("CA-SCL", 64, 40, 29, 16, "ties"): (-0.5, 0, 96),
    ("CA-SCL", 128, 70, 46, 13, "awgn"): (-0.5, 0, 96),
    ("CA-SCL", 128, 70, 46, 13, "ties"): (-0.5, 0, 96),
    ("CA-SCL", 256, 128, 104, 8, "awgn"): (0.0, 0, 96),
    ("CA-SCL", 256, 128, 104, 8, "ties"): (1.0, 0, 96),
    ("CA-SCL", 1024, 512, 488, 8, "awgn"): (2.0, 1, 192),
    ("CA-SCL", 1024, 512, 488, 8, "ties"): (0.0, 0, 384),
    ("CA-SCL", 128, 64, 40, 32, "awgn"): (-0.5, 0, 96),
    ("CA-SCL", 128, 64, 40, 32, "ties"): (-0.5, 0, 96),
    ("CA-SCL-LUT", 32, 30, 6, 2, "minsum"): (1.0, 0, 96),
    ("CA-FastSCL-LUT", 32, 30, 6, 2, "minsum"): (1.0, 0, 96),
    ("CA-SCL-LUT", 1024, 512, 488, 8, "minsum"): (1.0, 0, 384),
    ("CA-FastSCL-LUT", 1024, 512, 488, 8, "minsum"): (1.0, 1, 384),
    ("CA-SCL-LUT", 1024, 512, 500, 8, "minsum"): (2.5, 0, 384),
    ("CA-FastSCL-LUT", 1024, 512, 500, 8, "minsum"): (1.5, 1, 192),
    ("CA-SCL-LUT", 256, 128, 104, 8, "minsum", 97): (1.5, 2, 97),
    ("CA-SCL-LUT", 256, 128, 104, 8, "minsum", 517): (-0.5, 0, 517),
    ("CA-SCL", 128, 64, 40, 8, "awgn", 517): (-0.5, 0, 517),
}


def _ca(kind, N, A, crc_n, L, tables, K=0, B=0, **kw):
    K = K or A + crc_n
    ebn0, seed, b = CA_INPUTS[(kind, N, K, A, L, tables, B) if B else (kind, N, K, A, L, tables)]
    unmet = "late,mask" if tables == "random" else "ties" if (L, tables) == (2, "minsum") else ""
    return Case(kind, N, K, L, tables, A=A, crc_n=crc_n, ebn0=ebn0, seed=seed, B=b, unmet=unmet, **kw)


# N, A, crc_n, L, tables, K: the codes of test_gpu_parity.CA_CASES
CA_ROWS = [
    (32, 6, 24, 2, "minsum", 30),
    (64, 20, 24, 4, "minsum", 44),
    (128, 40, 24, 8, "minsum", 64),
    (128, 40, 24, 8, "random", 64),
    (128, 40, 24, 16, "random", 64),
    (256, 100, 24, 12, "minsum", 124),
    (256, 100, 11, 8, "minsum", 111),  # CRC11
    (512, 230, 24, 3, "minsum", 254),
    (1024, 488, 24, 8, "minsum", 512),
    (1024, 500, 24, 8, "minsum", 512),  # K - A = 12 < crc_n: the first 12 check bits are compared
]


def _cases():
    out = []
    # SCL-LUT / FastSCL-LUT without CRC: (256, 128, 8) is the first split tail (N / 32 >= lanes per frame)
    for N, K, L in [(4, 2, 2), (16, 8, 4), (64, 20, 5), (128, 64, 8), (256, 128, 8), (256, 128, 7), (512, 256, 3),
                    (1024, 512, 8)]:
        for tables in ("random", "continuous", "minsum"):
            for kind in ("SCL-LUT", "FastSCL-LUT"):
                for engine in ("auto", "generic"):
                    out.append(Case(kind, N, K, L, tables, engine, B=48 if (N, tables) == (1024, "minsum") else _b(N),
                                    unmet="ties" if (N, tables) == (4, "minsum") else ""))
    # K % 4 != 0 (byte output path), N < 32 (the root word's mask)
    for N, K, L in [(16, 7, 4), (64, 21, 8)]:
        for kind in ("SCL-LUT", "FastSCL-LUT"):
            for engine in ("auto", "generic"):
                out.append(Case(kind, N, K, L, "random", engine))
    # lane groups of 16
    for N, K in [(128, 64), (512, 256)]:
        for L in (9, 16):
            out.append(Case("SCL-LUT", N, K, L, "random"))
            out.append(_ca("CA-SCL-LUT", N, K - 24, 24, L, "minsum"))
    for N, K in [(128, 64), (512, 200)]:  # (512, 256) has an R1 node of 64 elements: not served at L > 8
        for L in (9, 12, 16):
            out.append(Case("FastSCL-LUT", N, K, L, "random", "fast"))
            out.append(_ca("CA-FastSCL-LUT", N, K - 24, 24, L, "minsum", engine="fast"))
    # R1L twins: R1 nodes beyond the LDS tail
    for N, K, L in [(512, 420, 5), (1024, 900, 8)] + R1L_BELOW_8:
        for env in (_env(), _env(QPD_LDS_BUDGET="256")):
            out.append(Case("FastSCL-LUT", N, K, L, "random", "fast", env, B=48))
    N, K, L = R1L_BELOW_8[0]
    out.append(Case("FastSCL-LUT", N, K, L, "random", "fast", _env(QPD_SETS="1"), B=48))
    out.append(Case("FastSCL-LUT", 1024, 900, 8, "random", "fast", _env(QPD_SETS="1"), B=48))
    # both pointer-word layouts: SCL-LUT's op list fits one word per path up to N = 2048 and not at 4096
    # (compact_pointer_fields); FastSCL-LUT takes one word with L = 8, two sets and no large R1 node (min-sum
    # tables at N = 1024, above), and two when told to
    for N in (2048, 4096):
        out.append(Case("SCL-LUT", N, N // 2, 8, "random", "fast", B=16))
    out.append(Case("SCL-LUT", 128, 64, 8, "random", "fast", _env(QPD_NO_PW1="1")))
    out.append(Case("FastSCL-LUT", 1024, 512, 8, "minsum", "fast", _env(QPD_NO_PW1="1"), B=48))
    out.append(Case("FastSCL-LUT", 128, 64, 12, "random", "fast", _env(QPD_NO_PW1="1")))
    out.append(Case("SCL-LUT", 128, 64, 16, "random", "fast", _env(QPD_NO_PW1="1")))
    # one frame set per wave
    for kind, N, K, L, tables in [("FastSCL-LUT", 256, 128, 8, "minsum"), ("FastSCL-LUT", 256, 128, 5, "random"),
                                  ("FastSCL-LUT", 128, 64, 12, "random"), ("SCL-LUT", 128, 64, 12, "random")]:
        out.append(Case(kind, N, K, L, tables, "fast", _env(QPD_SETS="1")))
    out.append(Case("FastSCL-LUT", 128, 64, 12, "random", "fast", _env(QPD_NO_PW1="1", QPD_SETS="1")))
    # planner modes
    for env in (_env(), _env(QPD_NO_PFX="1"), _env(QPD_NO_PRE="1"), _env(QPD_PFX1B="1"), _env(QPD_SETS="1"),
                _env(QPD_SETS="2"), _env(QPD_LDS_BUDGET="256")):
        out.append(Case("SCL-LUT", 1024, 512, 8, "random", "fast", env, B=24))
        out.append(_ca("CA-SCL-LUT", 256, 104, 24, 4, "minsum", engine="fast", env=env))
    # CRC-aided LUT kinds: the rows of test_gpu_parity.CA_CASES (CA-FastSCL-LUT is undefined where the code's
    # root is a special node: special_root)
    for N, A, crc_n, L, tables, K in CA_ROWS:
        for kind in ("CA-SCL-LUT", "CA-FastSCL-LUT"):
            for engine in ("auto", "generic"):
                if not special_root(Case(kind, N, K, L)):
                    out.append(_ca(kind, N, A, crc_n, L, tables, K=K, engine=engine))
    # the generic engine beyond the fast engine's reach
    for kind in ("SCL-LUT", "FastSCL-LUT"):
        out.append(Case(kind, 32, 16, 8, "perelem", "generic"))
        out.append(Case(kind, 128, 80, 21, "random", "generic"))
        out.append(Case(kind, 256, 128, 32, "random", "generic"))
        for v in (3, 17, 256):
            out.append(Case(kind, 64, 32, 8, "random", "generic", v=v, mask="random1"))
    # float list kinds (the generic kernel, narrow and wide lists)
    for N, K, L in [(8, 4, 3), (64, 40, 16), (128, 70, 13), (256, 128, 8), (1024, 512, 8), (128, 64, 32)]:
        for style in ("awgn", "ties"):
            for kind in ("SCL", "FastSCL", "SCL-Uniform", "SCL-Lloyd"):
                out.append(Case(kind, N, K, L, style, "generic", B=_b(N)))
            if K >= 35:  # CA-SCL needs A + crc_n <= K
                crc_n = 24 if K >= 64 else 11
                out.append(_ca("CA-SCL", N, K - crc_n, crc_n, L, style, K=K, engine="generic"))
    # launch seams: several launches per call, grid-stride rounds, partial waves
    for dtype in ("i32", "u8"):
        out.append(_ca("CA-SCL-LUT", 256, 104, 24, 8, "minsum", B=97, engine="fast", env=_env(QPD_PRE_CHUNK="32"), dtype=dtype))
        out.append(Case("SCL-LUT", 256, 128, 4, "random", "fast", _env(QPD_PRE_CHUNK="32"), B=97, dtype=dtype))
    out.append(Case("SCL-LUT", 128, 64, 8, "random", "generic", _env(QPD_U8_CHUNK="32"), B=97, dtype="u8"))
    out.append(Case("SCL-LUT", 128, 64, 8, "random", "fast", _env(QPD_NO_PRE="1", QPD_U8_CHUNK="32"), B=97, dtype="u8"))
    for kind, engine in (("SCL-LUT", "fast"), ("FastSCL-LUT", "fast"), ("SCL-LUT", "generic")):
        out.append(Case(kind, 256, 128, 8, "random", engine, B=517, max_waves=3))
        out.append(Case(kind, 256, 128, 8, "random", engine, B=1))
        out.append(Case(kind, 256, 128, 8, "random", engine, B=37))  # no multiple of any frames_per_wave (8, 16)
    out.append(_ca("CA-SCL-LUT", 256, 104, 24, 8, "minsum", B=517, engine="fast", max_waves=3))
    out.append(Case("SCL", 128, 64, 8, "ties", "generic", B=517, max_waves=3))
    out.append(_ca("CA-SCL", 128, 40, 24, 8, "awgn", B=517, engine="generic", max_waves=3))
    ids = [c.id for c in out]
    assert len(set(ids)) == len(ids), sorted(i for i in ids if ids.count(i) > 1)
    return out


# FastSCL-LUT codes (N, K, L) with L < 8 whose plan has an R1 node that needs r1_large: found with the planner
# harness of tests/test_plan.py; the first also at one frame set per wave
R1L_BELOW_8 = [(256, 220, 5)]

CASES = _cases()



# (engine, lanes_per_frame, frames_per_wave, fast_variant, prefix_ops > 0) per case id, in the order of CASES:
# planned on the CPU with the harness of tests/test_plan.py when the case was written
EXPECT = {
    'SCL-LUT-4-2-2-random-auto': (2, 2, 64, 0, False),
    'SCL-LUT-4-2-2-random-generic': (1, 2, 32, 0, False),
    'FastSCL-LUT-4-2-2-random-auto': (2, 2, 64, 0, False),
    'FastSCL-LUT-4-2-2-random-generic': (1, 2, 32, 0, False),
    'SCL-LUT-4-2-2-continuous-auto': (2, 2, 64, 0, False),
    'SCL-LUT-4-2-2-continuous-generic': (1, 2, 32, 0, False),
    'FastSCL-LUT-4-2-2-continuous-auto': (2, 2, 64, 0, False),
    'FastSCL-LUT-4-2-2-continuous-generic': (1, 2, 32, 0, False),
    'SCL-LUT-4-2-2-minsum-auto': (2, 2, 64, 0, False),
    'SCL-LUT-4-2-2-minsum-generic': (1, 2, 32, 0, False),
    'FastSCL-LUT-4-2-2-minsum-auto': (2, 2, 64, 0, False),
    'FastSCL-LUT-4-2-2-minsum-generic': (1, 2, 32, 0, False),
    'SCL-LUT-16-8-4-random-auto': (2, 4, 32, 1, False),
    'SCL-LUT-16-8-4-random-generic': (1, 4, 16, 0, False),
    'FastSCL-LUT-16-8-4-random-auto': (2, 4, 32, 0, False),
    'FastSCL-LUT-16-8-4-random-generic': (1, 4, 16, 0, False),
    'SCL-LUT-16-8-4-continuous-auto': (2, 4, 32, 1, False),
    'SCL-LUT-16-8-4-continuous-generic': (1, 4, 16, 0, False),
    'FastSCL-LUT-16-8-4-continuous-auto': (2, 4, 32, 0, False),
    'FastSCL-LUT-16-8-4-continuous-generic': (1, 4, 16, 0, False),
    'SCL-LUT-16-8-4-minsum-auto': (2, 4, 32, 1, False),
    'SCL-LUT-16-8-4-minsum-generic': (1, 4, 16, 0, False),
    'FastSCL-LUT-16-8-4-minsum-auto': (2, 4, 32, 0, False),
    'FastSCL-LUT-16-8-4-minsum-generic': (1, 4, 16, 0, False),
    'SCL-LUT-64-20-5-random-auto': (2, 8, 16, 1, True),
    'SCL-LUT-64-20-5-random-generic': (1, 8, 8, 0, False),
    'FastSCL-LUT-64-20-5-random-auto': (2, 8, 16, 0, False),
    'FastSCL-LUT-64-20-5-random-generic': (1, 8, 8, 0, False),
    'SCL-LUT-64-20-5-continuous-auto': (2, 8, 16, 1, True),
    'SCL-LUT-64-20-5-continuous-generic': (1, 8, 8, 0, False),
    'FastSCL-LUT-64-20-5-continuous-auto': (2, 8, 16, 0, False),
    'FastSCL-LUT-64-20-5-continuous-generic': (1, 8, 8, 0, False),
    'SCL-LUT-64-20-5-minsum-auto': (2, 8, 16, 1, True),
    'SCL-LUT-64-20-5-minsum-generic': (1, 8, 8, 0, False),
    'FastSCL-LUT-64-20-5-minsum-auto': (2, 8, 16, 0, False),
    'FastSCL-LUT-64-20-5-minsum-generic': (1, 8, 8, 0, False),
    'SCL-LUT-128-64-8-random-auto': (2, 8, 16, 1, True),
    'SCL-LUT-128-64-8-random-generic': (1, 8, 8, 0, False),
    'FastSCL-LUT-128-64-8-random-auto': (2, 8, 16, 2, False),
    'FastSCL-LUT-128-64-8-random-generic': (1, 8, 8, 0, False),
    'SCL-LUT-128-64-8-continuous-auto': (2, 8, 16, 1, True),
    'SCL-LUT-128-64-8-continuous-generic': (1, 8, 8, 0, False),
    'FastSCL-LUT-128-64-8-continuous-auto': (2, 8, 16, 2, False),
    'FastSCL-LUT-128-64-8-continuous-generic': (1, 8, 8, 0, False),
    'SCL-LUT-128-64-8-minsum-auto': (2, 8, 16, 1, True),
    'SCL-LUT-128-64-8-minsum-generic': (1, 8, 8, 0, False),
    'FastSCL-LUT-128-64-8-minsum-auto': (2, 8, 16, 1, False),
    'FastSCL-LUT-128-64-8-minsum-generic': (1, 8, 8, 0, False),
    'SCL-LUT-256-128-8-random-auto': (2, 8, 16, 1, True),
    'SCL-LUT-256-128-8-random-generic': (1, 8, 8, 0, False),
    'FastSCL-LUT-256-128-8-random-auto': (2, 8, 16, 2, False),
    'FastSCL-LUT-256-128-8-random-generic': (1, 8, 8, 0, False),
    'SCL-LUT-256-128-8-continuous-auto': (2, 8, 16, 1, True),
    'SCL-LUT-256-128-8-continuous-generic': (1, 8, 8, 0, False),
    'FastSCL-LUT-256-128-8-continuous-auto': (2, 8, 16, 2, False),
    'FastSCL-LUT-256-128-8-continuous-generic': (1, 8, 8, 0, False),
    'SCL-LUT-256-128-8-minsum-auto': (2, 8, 16, 1, True),
    'SCL-LUT-256-128-8-minsum-generic': (1, 8, 8, 0, False),
    'FastSCL-LUT-256-128-8-minsum-auto': (2, 8, 16, 1, False),
    'FastSCL-LUT-256-128-8-minsum-generic': (1, 8, 8, 0, False),
    'SCL-LUT-256-128-7-random-auto': (2, 8, 16, 1, True),
    'SCL-LUT-256-128-7-random-generic': (1, 8, 8, 0, False),
    'FastSCL-LUT-256-128-7-random-auto': (2, 8, 16, 0, False),
    'FastSCL-LUT-256-128-7-random-generic': (1, 8, 8, 0, False),
    'SCL-LUT-256-128-7-continuous-auto': (2, 8, 16, 1, True),
    'SCL-LUT-256-128-7-continuous-generic': (1, 8, 8, 0, False),
    'FastSCL-LUT-256-128-7-continuous-auto': (2, 8, 16, 0, False),
    'FastSCL-LUT-256-128-7-continuous-generic': (1, 8, 8, 0, False),
    'SCL-LUT-256-128-7-minsum-auto': (2, 8, 16, 1, True),
    'SCL-LUT-256-128-7-minsum-generic': (1, 8, 8, 0, False),
    'FastSCL-LUT-256-128-7-minsum-auto': (2, 8, 16, 0, False),
    'FastSCL-LUT-256-128-7-minsum-generic': (1, 8, 8, 0, False),
    'SCL-LUT-512-256-3-random-auto': (2, 4, 32, 1, True),
    'SCL-LUT-512-256-3-random-generic': (1, 4, 16, 0, False),
    'FastSCL-LUT-512-256-3-random-auto': (2, 4, 32, 2, False),
    'FastSCL-LUT-512-256-3-random-generic': (1, 4, 16, 0, False),
    'SCL-LUT-512-256-3-continuous-auto': (2, 4, 32, 1, True),
    'SCL-LUT-512-256-3-continuous-generic': (1, 4, 16, 0, False),
    'FastSCL-LUT-512-256-3-continuous-auto': (2, 4, 32, 2, False),
    'FastSCL-LUT-512-256-3-continuous-generic': (1, 4, 16, 0, False),
    'SCL-LUT-512-256-3-minsum-auto': (2, 4, 32, 1, True),
    'SCL-LUT-512-256-3-minsum-generic': (1, 4, 16, 0, False),
    'FastSCL-LUT-512-256-3-minsum-auto': (2, 4, 32, 2, False),
    'FastSCL-LUT-512-256-3-minsum-generic': (1, 4, 16, 0, False),
    'SCL-LUT-1024-512-8-random-auto-B24': (2, 8, 16, 1, True),
    'SCL-LUT-1024-512-8-random-generic-B24': (1, 8, 8, 0, False),
    'FastSCL-LUT-1024-512-8-random-auto-B24': (2, 8, 16, 2, False),
    'FastSCL-LUT-1024-512-8-random-generic-B24': (1, 8, 8, 0, False),
    'SCL-LUT-1024-512-8-continuous-auto-B24': (2, 8, 16, 1, True),
    'SCL-LUT-1024-512-8-continuous-generic-B24': (1, 8, 8, 0, False),
    'FastSCL-LUT-1024-512-8-continuous-auto-B24': (2, 8, 16, 2, False),
    'FastSCL-LUT-1024-512-8-continuous-generic-B24': (1, 8, 8, 0, False),
    'SCL-LUT-1024-512-8-minsum-auto-B48': (2, 8, 16, 1, True),
    'SCL-LUT-1024-512-8-minsum-generic-B48': (1, 8, 8, 0, False),
    'FastSCL-LUT-1024-512-8-minsum-auto-B48': (2, 8, 16, 1, False),
    'FastSCL-LUT-1024-512-8-minsum-generic-B48': (1, 8, 8, 0, False),
    'SCL-LUT-16-7-4-random-auto': (2, 4, 32, 1, False),
    'SCL-LUT-16-7-4-random-generic': (1, 4, 16, 0, False),
    'FastSCL-LUT-16-7-4-random-auto': (2, 4, 32, 0, False),
    'FastSCL-LUT-16-7-4-random-generic': (1, 4, 16, 0, False),
    'SCL-LUT-64-21-8-random-auto': (2, 8, 16, 1, True),
    'SCL-LUT-64-21-8-random-generic': (1, 8, 8, 0, False),
    'FastSCL-LUT-64-21-8-random-auto': (2, 8, 16, 2, False),
    'FastSCL-LUT-64-21-8-random-generic': (1, 8, 8, 0, False),
    'SCL-LUT-128-64-9-random-auto': (2, 16, 8, 1, True),
    'CA-SCL-LUT-128-64-9-minsum-auto-A40c24': (2, 16, 8, 1, True),
    'SCL-LUT-128-64-16-random-auto': (2, 16, 8, 1, True),
    'CA-SCL-LUT-128-64-16-minsum-auto-A40c24': (2, 16, 8, 1, True),
    'SCL-LUT-512-256-9-random-auto': (2, 16, 8, 1, True),
    'CA-SCL-LUT-512-256-9-minsum-auto-A232c24-B384': (2, 16, 8, 1, True),
    'SCL-LUT-512-256-16-random-auto': (2, 16, 8, 1, True),
    'CA-SCL-LUT-512-256-16-minsum-auto-A232c24': (2, 16, 8, 1, True),
    'FastSCL-LUT-128-64-9-random-fast': (2, 16, 8, 1, False),
    'CA-FastSCL-LUT-128-64-9-minsum-fast-A40c24': (2, 16, 8, 1, False),
    'FastSCL-LUT-128-64-12-random-fast': (2, 16, 8, 1, False),
    'CA-FastSCL-LUT-128-64-12-minsum-fast-A40c24': (2, 16, 8, 1, False),
    'FastSCL-LUT-128-64-16-random-fast': (2, 16, 8, 1, False),
    'CA-FastSCL-LUT-128-64-16-minsum-fast-A40c24': (2, 16, 8, 1, False),
    'FastSCL-LUT-512-200-9-random-fast': (2, 16, 8, 0, False),
    'CA-FastSCL-LUT-512-200-9-minsum-fast-A176c24-B768': (2, 16, 8, 0, False),
    'FastSCL-LUT-512-200-12-random-fast': (2, 16, 8, 0, False),
    'CA-FastSCL-LUT-512-200-12-minsum-fast-A176c24-B384': (2, 16, 8, 0, False),
    'FastSCL-LUT-512-200-16-random-fast': (2, 16, 8, 0, False),
    'CA-FastSCL-LUT-512-200-16-minsum-fast-A176c24-B768': (2, 16, 8, 0, False),
    'FastSCL-LUT-512-420-5-random-fast-B48': (2, 8, 16, 0, False),
    'FastSCL-LUT-512-420-5-random-fast-B48-LDS_BUDGET256': (2, 8, 16, 0, False),
    'FastSCL-LUT-1024-900-8-random-fast-B48': (2, 8, 16, 2, False),
    'FastSCL-LUT-1024-900-8-random-fast-B48-LDS_BUDGET256': (2, 8, 16, 2, False),
    'FastSCL-LUT-256-220-5-random-fast-B48': (2, 8, 16, 2, False),
    'FastSCL-LUT-256-220-5-random-fast-B48-LDS_BUDGET256': (2, 8, 16, 2, False),
    'FastSCL-LUT-256-220-5-random-fast-B48-SETS1': (2, 8, 8, 2, False),
    'FastSCL-LUT-1024-900-8-random-fast-B48-SETS1': (2, 8, 8, 2, False),
    'SCL-LUT-2048-1024-8-random-fast-B16': (2, 8, 16, 1, True),
    'SCL-LUT-4096-2048-8-random-fast-B16': (2, 8, 16, 0, True),
    'SCL-LUT-128-64-8-random-fast-NO_PW11': (2, 8, 16, 0, True),
    'FastSCL-LUT-1024-512-8-minsum-fast-B48-NO_PW11': (2, 8, 16, 0, False),
    'FastSCL-LUT-128-64-12-random-fast-NO_PW11': (2, 16, 8, 0, False),
    'SCL-LUT-128-64-16-random-fast-NO_PW11': (2, 16, 8, 0, True),
    'FastSCL-LUT-256-128-8-minsum-fast-SETS1': (2, 8, 8, 0, False),
    'FastSCL-LUT-256-128-5-random-fast-SETS1': (2, 8, 8, 0, False),
    'FastSCL-LUT-128-64-12-random-fast-SETS1': (2, 16, 4, 1, False),
    'SCL-LUT-128-64-12-random-fast-SETS1': (2, 16, 4, 1, True),
    'FastSCL-LUT-128-64-12-random-fast-NO_PW11-SETS1': (2, 16, 4, 0, False),
    'SCL-LUT-1024-512-8-random-fast-B24': (2, 8, 16, 1, True),
    'CA-SCL-LUT-256-128-4-minsum-fast-A104c24': (2, 4, 32, 1, True),
    'SCL-LUT-1024-512-8-random-fast-B24-NO_PFX1': (2, 8, 16, 1, False),
    'CA-SCL-LUT-256-128-4-minsum-fast-A104c24-NO_PFX1': (2, 4, 32, 1, False),
    'SCL-LUT-1024-512-8-random-fast-B24-NO_PRE1': (2, 8, 16, 0, False),
    'CA-SCL-LUT-256-128-4-minsum-fast-A104c24-NO_PRE1': (2, 4, 32, 0, False),
    'SCL-LUT-1024-512-8-random-fast-B24-PFX1B1': (2, 8, 16, 1, True),
    'CA-SCL-LUT-256-128-4-minsum-fast-A104c24-PFX1B1': (2, 4, 32, 1, True),
    'SCL-LUT-1024-512-8-random-fast-B24-SETS1': (2, 8, 8, 1, True),
    'CA-SCL-LUT-256-128-4-minsum-fast-A104c24-SETS1': (2, 4, 16, 1, True),
    'SCL-LUT-1024-512-8-random-fast-B24-SETS2': (2, 8, 16, 1, True),
    'CA-SCL-LUT-256-128-4-minsum-fast-A104c24-SETS2': (2, 4, 32, 1, True),
    'SCL-LUT-1024-512-8-random-fast-B24-LDS_BUDGET256': (2, 8, 16, 1, True),
    'CA-SCL-LUT-256-128-4-minsum-fast-A104c24-LDS_BUDGET256': (2, 4, 32, 1, True),
    'CA-SCL-LUT-32-30-2-minsum-auto-A6c24': (2, 2, 64, 1, True),
    'CA-SCL-LUT-32-30-2-minsum-generic-A6c24': (1, 2, 32, 0, False),
    'CA-FastSCL-LUT-32-30-2-minsum-auto-A6c24': (2, 2, 64, 0, False),
    'CA-FastSCL-LUT-32-30-2-minsum-generic-A6c24': (1, 2, 32, 0, False),
    'CA-SCL-LUT-64-44-4-minsum-auto-A20c24': (2, 4, 32, 1, True),
    'CA-SCL-LUT-64-44-4-minsum-generic-A20c24': (1, 4, 16, 0, False),
    'CA-FastSCL-LUT-64-44-4-minsum-auto-A20c24-B192': (2, 4, 32, 0, False),
    'CA-FastSCL-LUT-64-44-4-minsum-generic-A20c24-B192': (1, 4, 16, 0, False),
    'CA-SCL-LUT-128-64-8-minsum-auto-A40c24': (2, 8, 16, 1, True),
    'CA-SCL-LUT-128-64-8-minsum-generic-A40c24': (1, 8, 8, 0, False),
    'CA-FastSCL-LUT-128-64-8-minsum-auto-A40c24': (2, 8, 16, 1, False),
    'CA-FastSCL-LUT-128-64-8-minsum-generic-A40c24': (1, 8, 8, 0, False),
    'CA-SCL-LUT-128-64-8-random-auto-A40c24': (2, 8, 16, 1, True),
    'CA-SCL-LUT-128-64-8-random-generic-A40c24': (1, 8, 8, 0, False),
    'CA-FastSCL-LUT-128-64-8-random-auto-A40c24': (2, 8, 16, 2, False),
    'CA-FastSCL-LUT-128-64-8-random-generic-A40c24': (1, 8, 8, 0, False),
    'CA-SCL-LUT-128-64-16-random-auto-A40c24': (2, 16, 8, 1, True),
    'CA-SCL-LUT-128-64-16-random-generic-A40c24': (1, 16, 4, 0, False),
    'CA-FastSCL-LUT-128-64-16-random-auto-A40c24': (1, 16, 4, 0, False),
    'CA-FastSCL-LUT-128-64-16-random-generic-A40c24': (1, 16, 4, 0, False),
    'CA-SCL-LUT-256-124-12-minsum-auto-A100c24': (2, 16, 8, 1, True),
    'CA-SCL-LUT-256-124-12-minsum-generic-A100c24': (1, 16, 4, 0, False),
    'CA-FastSCL-LUT-256-124-12-minsum-auto-A100c24-B192': (1, 16, 4, 0, False),
    'CA-FastSCL-LUT-256-124-12-minsum-generic-A100c24-B192': (1, 16, 4, 0, False),
    'CA-SCL-LUT-256-111-8-minsum-auto-A100c11-B192': (2, 8, 16, 1, True),
    'CA-SCL-LUT-256-111-8-minsum-generic-A100c11-B192': (1, 8, 8, 0, False),
    'CA-FastSCL-LUT-256-111-8-minsum-auto-A100c11': (2, 8, 16, 1, False),
    'CA-FastSCL-LUT-256-111-8-minsum-generic-A100c11': (1, 8, 8, 0, False),
    'CA-SCL-LUT-512-254-3-minsum-auto-A230c24-B384': (2, 4, 32, 1, True),
    'CA-SCL-LUT-512-254-3-minsum-generic-A230c24-B384': (1, 4, 16, 0, False),
    'CA-FastSCL-LUT-512-254-3-minsum-auto-A230c24-B384': (2, 4, 32, 2, False),
    'CA-FastSCL-LUT-512-254-3-minsum-generic-A230c24-B384': (1, 4, 16, 0, False),
    'CA-SCL-LUT-1024-512-8-minsum-auto-A488c24-B384': (2, 8, 16, 1, True),
    'CA-SCL-LUT-1024-512-8-minsum-generic-A488c24-B384': (1, 8, 8, 0, False),
    'CA-FastSCL-LUT-1024-512-8-minsum-auto-A488c24-B384': (2, 8, 16, 1, False),
    'CA-FastSCL-LUT-1024-512-8-minsum-generic-A488c24-B384': (1, 8, 8, 0, False),
    'CA-SCL-LUT-1024-512-8-minsum-auto-A500c24-B384': (2, 8, 16, 1, True),
    'CA-SCL-LUT-1024-512-8-minsum-generic-A500c24-B384': (1, 8, 8, 0, False),
    'CA-FastSCL-LUT-1024-512-8-minsum-auto-A500c24-B192': (2, 8, 16, 1, False),
    'CA-FastSCL-LUT-1024-512-8-minsum-generic-A500c24-B192': (1, 8, 8, 0, False),
    'SCL-LUT-32-16-8-perelem-generic': (1, 8, 8, 0, False),
    'SCL-LUT-128-80-21-random-generic': (1, 32, 2, 0, False),
    'SCL-LUT-256-128-32-random-generic': (1, 32, 2, 0, False),
    'SCL-LUT-64-32-8-random-generic-v3-random1': (1, 8, 8, 0, False),
    'SCL-LUT-64-32-8-random-generic-v17-random1': (1, 8, 8, 0, False),
    'SCL-LUT-64-32-8-random-generic-v256-random1': (1, 8, 8, 0, False),
    'FastSCL-LUT-32-16-8-perelem-generic': (1, 8, 8, 0, False),
    'FastSCL-LUT-128-80-21-random-generic': (1, 32, 2, 0, False),
    'FastSCL-LUT-256-128-32-random-generic': (1, 32, 2, 0, False),
    'FastSCL-LUT-64-32-8-random-generic-v3-random1': (1, 8, 8, 0, False),
    'FastSCL-LUT-64-32-8-random-generic-v17-random1': (1, 8, 8, 0, False),
    'FastSCL-LUT-64-32-8-random-generic-v256-random1': (1, 8, 8, 0, False),
    'SCL-8-4-3-awgn-generic': (1, 4, 16, 0, False),
    'FastSCL-8-4-3-awgn-generic': (1, 4, 16, 0, False),
    'SCL-Uniform-8-4-3-awgn-generic': (1, 4, 16, 0, False),
    'SCL-Lloyd-8-4-3-awgn-generic': (1, 4, 16, 0, False),
    'SCL-8-4-3-ties-generic': (1, 4, 16, 0, False),
    'FastSCL-8-4-3-ties-generic': (1, 4, 16, 0, False),
    'SCL-Uniform-8-4-3-ties-generic': (1, 4, 16, 0, False),
    'SCL-Lloyd-8-4-3-ties-generic': (1, 4, 16, 0, False),
    'SCL-64-40-16-awgn-generic': (1, 16, 4, 0, False),
    'FastSCL-64-40-16-awgn-generic': (1, 16, 4, 0, False),
    'SCL-Uniform-64-40-16-awgn-generic': (1, 16, 4, 0, False),
    'SCL-Lloyd-64-40-16-awgn-generic': (1, 16, 4, 0, False),
    'CA-SCL-64-40-16-awgn-generic-A29c11': (1, 16, 4, 0, False),
    'SCL-64-40-16-ties-generic': (1, 16, 4, 0, False),
    'FastSCL-64-40-16-ties-generic': (1, 16, 4, 0, False),
    'SCL-Uniform-64-40-16-ties-generic': (1, 16, 4, 0, False),
    'SCL-Lloyd-64-40-16-ties-generic': (1, 16, 4, 0, False),
    'CA-SCL-64-40-16-ties-generic-A29c11': (1, 16, 4, 0, False),
    'SCL-128-70-13-awgn-generic': (1, 16, 4, 0, False),
    'FastSCL-128-70-13-awgn-generic': (1, 16, 4, 0, False),
    'SCL-Uniform-128-70-13-awgn-generic': (1, 16, 4, 0, False),
    'SCL-Lloyd-128-70-13-awgn-generic': (1, 16, 4, 0, False),
    'CA-SCL-128-70-13-awgn-generic-A46c24': (1, 16, 4, 0, False),
    'SCL-128-70-13-ties-generic': (1, 16, 4, 0, False),
    'FastSCL-128-70-13-ties-generic': (1, 16, 4, 0, False),
    'SCL-Uniform-128-70-13-ties-generic': (1, 16, 4, 0, False),
    'SCL-Lloyd-128-70-13-ties-generic': (1, 16, 4, 0, False),
    'CA-SCL-128-70-13-ties-generic-A46c24': (1, 16, 4, 0, False),
    'SCL-256-128-8-awgn-generic': (1, 8, 8, 0, False),
    'FastSCL-256-128-8-awgn-generic': (1, 8, 8, 0, False),
    'SCL-Uniform-256-128-8-awgn-generic': (1, 8, 8, 0, False),
    'SCL-Lloyd-256-128-8-awgn-generic': (1, 8, 8, 0, False),
    'CA-SCL-256-128-8-awgn-generic-A104c24': (1, 8, 8, 0, False),
    'SCL-256-128-8-ties-generic': (1, 8, 8, 0, False),
    'FastSCL-256-128-8-ties-generic': (1, 8, 8, 0, False),
    'SCL-Uniform-256-128-8-ties-generic': (1, 8, 8, 0, False),
    'SCL-Lloyd-256-128-8-ties-generic': (1, 8, 8, 0, False),
    'CA-SCL-256-128-8-ties-generic-A104c24': (1, 8, 8, 0, False),
    'SCL-1024-512-8-awgn-generic-B24': (1, 8, 8, 0, False),
    'FastSCL-1024-512-8-awgn-generic-B24': (1, 8, 8, 0, False),
    'SCL-Uniform-1024-512-8-awgn-generic-B24': (1, 8, 8, 0, False),
    'SCL-Lloyd-1024-512-8-awgn-generic-B24': (1, 8, 8, 0, False),
    'CA-SCL-1024-512-8-awgn-generic-A488c24-B192': (1, 8, 8, 0, False),
    'SCL-1024-512-8-ties-generic-B24': (1, 8, 8, 0, False),
    'FastSCL-1024-512-8-ties-generic-B24': (1, 8, 8, 0, False),
    'SCL-Uniform-1024-512-8-ties-generic-B24': (1, 8, 8, 0, False),
    'SCL-Lloyd-1024-512-8-ties-generic-B24': (1, 8, 8, 0, False),
    'CA-SCL-1024-512-8-ties-generic-A488c24-B384': (1, 8, 8, 0, False),
    'SCL-128-64-32-awgn-generic': (1, 32, 2, 0, False),
    'FastSCL-128-64-32-awgn-generic': (1, 32, 2, 0, False),
    'SCL-Uniform-128-64-32-awgn-generic': (1, 32, 2, 0, False),
    'SCL-Lloyd-128-64-32-awgn-generic': (1, 32, 2, 0, False),
    'CA-SCL-128-64-32-awgn-generic-A40c24': (1, 32, 2, 0, False),
    'SCL-128-64-32-ties-generic': (1, 32, 2, 0, False),
    'FastSCL-128-64-32-ties-generic': (1, 32, 2, 0, False),
    'SCL-Uniform-128-64-32-ties-generic': (1, 32, 2, 0, False),
    'SCL-Lloyd-128-64-32-ties-generic': (1, 32, 2, 0, False),
    'CA-SCL-128-64-32-ties-generic-A40c24': (1, 32, 2, 0, False),
    'CA-SCL-LUT-256-128-8-minsum-fast-A104c24-B97-PRE_CHUNK32': (2, 8, 16, 1, True),
    'SCL-LUT-256-128-4-random-fast-B97-PRE_CHUNK32': (2, 4, 32, 1, True),
    'CA-SCL-LUT-256-128-8-minsum-fast-A104c24-B97-u8-PRE_CHUNK32': (2, 8, 16, 1, True),
    'SCL-LUT-256-128-4-random-fast-B97-u8-PRE_CHUNK32': (2, 4, 32, 1, True),
    'SCL-LUT-128-64-8-random-generic-B97-u8-U8_CHUNK32': (1, 8, 8, 0, False),
    'SCL-LUT-128-64-8-random-fast-B97-u8-NO_PRE1-U8_CHUNK32': (2, 8, 16, 0, False),
    'SCL-LUT-256-128-8-random-fast-B517-mw3': (2, 8, 16, 1, True),
    'SCL-LUT-256-128-8-random-fast-B1': (2, 8, 16, 1, True),
    'SCL-LUT-256-128-8-random-fast-B37': (2, 8, 16, 1, True),
    'FastSCL-LUT-256-128-8-random-fast-B517-mw3': (2, 8, 16, 2, False),
    'FastSCL-LUT-256-128-8-random-fast-B1': (2, 8, 16, 2, False),
    'FastSCL-LUT-256-128-8-random-fast-B37': (2, 8, 16, 2, False),
    'SCL-LUT-256-128-8-random-generic-B517-mw3': (1, 8, 8, 0, False),
    'SCL-LUT-256-128-8-random-generic-B1': (1, 8, 8, 0, False),
    'SCL-LUT-256-128-8-random-generic-B37': (1, 8, 8, 0, False),
    'CA-SCL-LUT-256-128-8-minsum-fast-A104c24-B517-mw3': (2, 8, 16, 1, True),
    'SCL-128-64-8-ties-generic-B517-mw3': (1, 8, 8, 0, False),
    'CA-SCL-128-64-8-awgn-generic-A40c24-B517-mw3': (1, 8, 8, 0, False),
}
