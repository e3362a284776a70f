"""The case table of the Monte-Carlo generator's parity tests (csrc/qpd_mc.hip), shared by
tests/test_mc_cases.py (CPU: the table covers what it is made for) and
tests/test_gpu_mc_masks_quant.py (GPU): channel quantizers that make the generator's
guess-and-walk bisect_left walk, frozen masks that drive its info-bit deposit through every
branch, CRC tails shorter than the register, and seeds above 2^32.

The deposit, restated (mc_frames_kernel): the frame's K information bits lie in words
bw[0 .. kw) (kw = ceil(K / 32)) followed by two zero pad words bw[kw], bw[kw + 1]; the lane
of 16-bit half h of u word w = h / 2 reads bw[s >> 5] and bw[(s >> 5) + 1], with
s = info_pref[w] + (popcount of the word's low half, for the high half), shifts them right
by s & 31 and deposits popcount(half) bits.  `deposit_reads` computes exactly that from the
mask alone."""
import numpy as np

import code_masks as M
import llr_vectors as V
from quantized_decoder_polar_codes_amd import codes as C
from quantized_decoder_polar_codes_amd import montecarlo as MC

SEEDS = (424242, 0xDEADBEEF12345678, 2 ** 64 - 1)

# CA-SCL-LUT (crc_n = 24) on the PW code of N = 128: (K, A), K - A in {1, 8, 23, 24}, A on the
# byte grid (the 8-byte message stores) and off it
CRC_N = 24
CRC_CASES = ((65, 64), (61, 53), (63, 40), (61, 37), (64, 40))


# ---------------------------------------------------------------------------------------------
# channel quantizers
# ---------------------------------------------------------------------------------------------

def scrambled_lut(M_, q, rng):
    """M_ symbols of [0, q) such that neighbouring bins differ and, from three bins on, the
    sequence is not monotone: a result one bin off, or a search that lands on the wrong side
    of a run, shows in the symbol."""
    if M_ == 1:
        return np.array([q // 2], dtype=np.int32)
    if M_ == 2:
        return np.array([q - 1, 0], dtype=np.int32)
    while True:
        if M_ <= q:
            lut = rng.permutation(q)[:M_]
        else:
            lut = rng.integers(0, q, size=M_)
            for i in range(1, M_):
                while lut[i] == lut[i - 1]:
                    lut[i] = rng.integers(0, q)
        d = np.diff(lut)
        if (d != 0).all() and (d > 0).any() and (d < 0).any():
            return lut.astype(np.int32)


ADDED = ("clustered", "wide", "overflow", "allequal", "q256", "q300", "q2", "q3", "q8", "q15")
SYMBOL_MODE_ONLY = ("q300",)  # q > 256: no reconstruction table


def quantizers(lutgen=None):
    """{name: (edges, lut, q)}: llr_vectors.quantizers()'s five (``lutgen`` as there) and the ADDED ones."""
    out = dict(V.quantizers(lutgen))
    rng = np.random.default_rng(20260)
    # 255 inner edges inside [0, 1e-3] between outer edges +-50: the guess from the mean bin
    # width (100 / 256) is up to half the table away from the bin, on either side
    e = np.concatenate([[-50.0], np.sort(rng.uniform(0.0, 1e-3, size=255)), [50.0]])
    out["clustered"] = (e, scrambled_lut(256, 16, rng), 16)
    # every LLR guesses the middle bin
    e = np.concatenate([[-1e300], np.sort(rng.normal(0, 6, size=255)), [1e300]])
    out["wide"] = (e, scrambled_lut(256, 16, rng), 16)
    # hi - lo = inf: inv_w = 0, the guess is bin 1
    e = np.concatenate([[-1.5e308], np.sort(rng.normal(0, 4, size=15)), [1.5e308]])
    out["overflow"] = (e, scrambled_lut(16, 16, rng), 16)
    out["allequal"] = (np.array([1.0, 1.0]), scrambled_lut(1, 3, rng), 3)
    out["q256"] = (0.125 * (np.arange(257, dtype=np.float64) - 128), scrambled_lut(256, 256, rng), 256)
    out["q300"] = (np.array([-1.0, 0.5, 2.0]), np.array([0, 299], dtype=np.int32), 300)
    for v in (2, 3, 8, 15):
        e, _ = MC.uniform_channel_quantizer(v, 0.5)
        out[f"q{v}"] = (e, scrambled_lut(v, v, rng), v)
    return out


def uniform_q(q):
    """The table's uniform quantizer of q symbols (the `uniform` entry for 16)."""
    return quantizers()["uniform" if q == 16 else f"q{q}"]


# ---------------------------------------------------------------------------------------------
# frozen masks
# ---------------------------------------------------------------------------------------------

def pw_big(N, K):
    """A frozen set beyond the 5G sequence: the K largest-weight positions as information bits."""
    w = np.array([bin(i).count("1") for i in range(N)])
    order = np.lexsort((np.arange(N), w))
    fm = np.ones(N, dtype=np.int64)
    fm[order[N - K:]] = 0
    return fm


BIG = (4096, 2072)  # nw = 128 words, kw + 2 = 67 message words: every per-word loop goes round more than once


def masks():
    """[(family, name, frozen mask)]; families: edge, block, random, pw, big."""
    out = []
    for N in (16, 64):
        for name in M.EDGE_NAMES:
            out.append(("edge", f"{name}-{N}", M.named_mask(N, name)))
    for N in (64, 256):
        for s in M.BLOCK_SEEDS[N]:
            out.append(("block", f"block{s}-{N}", M.block_mask(N, s)))
    for N, K, s in M.RANDOM_CASES:
        out.append(("random", f"random{s}-{N}-{K}", M.random_mask(N, K, s)))
    for N in (2, 4, 8, 32):
        out.append(("pw", f"pw-{N}", np.asarray(C.construct_pw(N, N // 2)[2], dtype=np.int64)))
    out.append(("big", f"big-{BIG[0]}", pw_big(*BIG)))
    return out


def mask_ids():
    return [name for _, name, _ in masks()]


def deposit_reads(fm):
    """[(half, s, popcount(half), (first word read, second word read))] of every 16-bit half, as the kernel
    computes them from info_mask / info_pref (see the module docstring)."""
    info = np.asarray(fm).reshape(-1) == 0
    N = info.size
    nw = (N + 31) >> 5
    bits = np.zeros(32 * nw, dtype=np.int64)
    bits[:N] = info
    words = bits.reshape(nw, 32)
    pref = np.concatenate([[0], np.cumsum(words.sum(1))[:-1]])
    out = []
    for h in range(2 * nw):
        w = h >> 1
        lo = int(words[w, :16].sum())
        pop = int(words[w, 16:].sum()) if h & 1 else lo
        s = int(pref[w]) + (lo if h & 1 else 0)
        out.append((h, s, pop, (s >> 5, (s >> 5) + 1)))
    return out


def properties(fm):
    """What a mask makes the deposit (and the loops around it) do: a set of names."""
    fm = np.asarray(fm).reshape(-1)
    N, K = fm.size, int((fm == 0).sum())
    nw, kw = (N + 31) >> 5, (K + 31) >> 5
    reads = deposit_reads(fm)
    p = set()
    for h, s, pop, (a, b) in reads:
        if pop == 16:
            p.add("half16")
        if pop == 0:
            p.add("half0")
        if s > 0 and s & 31 == 0:
            p.add("shift0")
        if s & 31 > 16:
            p.add("shift>16")
        if (s & 31) and (s & 31) + pop > 32:
            p.add("straddle")  # the deposited bits come from both words of the funnel
        if kw in (a, b):
            p.add("pad_kw")
        if kw + 1 in (a, b):
            p.add("pad_kw+1")
        assert b <= kw + 1, "a read past the two pad words"
    for w in range(nw):
        if reads[2 * w][2] + reads[2 * w + 1][2] == 0:
            p.add("word0")
    if K == N:
        p.add("K=N")
    if K == 1:
        p.add("K=1")
    if nw > 64:
        p.add("nw>64")
    if kw + 2 > 64:
        p.add("kw+2>64")
    if N < 32:
        p.add("N<32")
    if N == 2:
        p.add("N=2")
    if K & 7:
        p.add("K%8")  # message rows off the 8-byte grid: byte stores
    return p


def shift_count(fm):
    """How many different funnel shifts (s & 31) the mask's non-empty halves use."""
    return len({s & 31 for _, s, pop, _ in deposit_reads(fm) if pop})


# What each family is in the table for (tests/test_mc_cases.py asserts it family by family, so that a family
# cannot leave the table unnoticed): names of `properties`, all met by ONE mask where a tuple groups them.
PURPOSE = {
    "edge": ["half16", "half0", "word0", "shift0", "shift>16", "pad_kw", "pad_kw+1", "K=N", "K=1"],
    "block": [("half0", "half16", "straddle", "shift>16", "K%8")],
    "random": [("straddle", "shift>16")],
    "pw": ["N<32", "N=2", "K%8"],
    "big": [("nw>64", "kw+2>64", "straddle", "word0", "shift0")],
}
MIN_SHIFTS = {"block": 8, "random": 16, "big": 32}  # different funnel shifts in one mask of the family
