"""Frozen masks that no reliability order produces, for the parity tests.

construct_pw and the BEC construction give nested reliability orders: position
0 is never information, position N-1 never frozen, an R1 node is never followed
by an R0 node, and the special nodes come only in the few sizes and orders those
codes contain.  qpd_create accepts any 0/1 mask with K zeros, and the mask
drives the frozen-prefix stages, the register-resident bottom subtrees, the
folded special nodes and the R1 argsort paths; the generators here reach what
the nested orders leave out.  Every generator is deterministic per seed and
returns an int64 mask, 1 = frozen (the convention of codes.construct_pw).

test_code_masks.py asserts that the seeds chosen below cover what they are
chosen for.
"""
import numpy as np

from quantized_decoder_polar_codes_amd import codes as C

BLOCK_KINDS = ("R0", "R1", "REP", "SPC", "RND")
NODE_NAMES = {C.R0: "R0", C.R1: "R1", C.REP: "REP", C.SPC: "SPC"}

# The seeds of the parity tests: {N: seeds}.  BLOCK_SEEDS[256][0] holds a 64-element R1 node (the case of the
# schedule-switch test), BLOCK_SEEDS[1024] is the one long case.
BLOCK_SEEDS = {64: (2, 6, 7, 8, 11), 256: (5, 3, 9, 10), 1024: (5,)}
RANDOM_CASES = ((128, 64, 1), (512, 256, 2))  # (N, K, seed)


def random_mask(N, K, seed):
    """K information positions chosen uniformly among the N."""
    fm = np.ones(N, dtype=np.int64)
    fm[np.random.default_rng(seed).choice(N, size=K, replace=False)] = 0
    return fm


def block_mask(N, seed):
    """Aligned power-of-two blocks, left to right, each an R0, R1, REP (only the last leaf information), SPC
    (only the first leaf frozen) or random block.  Sizes are 1 .. 64, capped at N/2 and by the alignment of the
    position; the draw takes the largest size that fits with probability 1/2, the next one with 1/4, and so on
    (a uniform draw over the sizes gives almost only blocks of up to 4: a small block leaves the walk at a
    position aligned to nothing larger)."""
    rng = np.random.default_rng(seed)
    fm = np.ones(N, dtype=np.int64)
    pos = 0
    while pos < N:
        cap = min(64, max(1, N // 2))
        fit = cap if pos == 0 else min(cap, pos & -pos)  # the largest aligned block at pos
        sizes = [fit >> i for i in range(fit.bit_length())]  # fit, fit/2, .., 1
        w = np.array([0.5 ** (i + 1) for i in range(len(sizes))])
        w[-1] *= 2  # the tail of the geometric draw
        s = int(sizes[rng.choice(len(sizes), p=w / w.sum())])
        kind = BLOCK_KINDS[rng.integers(len(BLOCK_KINDS))]
        if kind == "R1":
            fm[pos:pos + s] = 0
        elif kind == "REP":
            fm[pos + s - 1] = 0
        elif kind == "SPC":
            fm[pos + (1 if s > 1 else 0):pos + s] = 0
        elif kind == "RND":
            fm[pos:pos + s] = rng.integers(0, 2, size=s)
        pos += s
    return fm


def _from_info(N, info):
    fm = np.ones(N, dtype=np.int64)
    fm[np.asarray(sorted(set(int(i) for i in info if 0 <= i < N)), dtype=np.int64)] = 0
    return fm


def edge_masks(N):
    """Named masks at the edges of what qpd_create accepts (N >= 8)."""
    out = {}
    out["info0"] = _from_info(N, [0, N // 4 + 1, N // 2, N // 2 + 3, N - 2])  # an empty frozen prefix
    fm = np.zeros(N, dtype=np.int64)
    fm[[N // 4, N - 1]] = 1
    out["frozen_last"] = fm
    out["K1_mid"] = _from_info(N, [N // 2 + 1])
    fm = np.zeros(N, dtype=np.int64)
    fm[N // 2 - 1] = 1
    out["KN-1_mid"] = fm
    out["all_info"] = np.zeros(N, dtype=np.int64)
    out["alt10"] = (np.arange(N) % 2 == 0).astype(np.int64)  # frozen, information, frozen, ..
    out["alt01"] = (np.arange(N) % 2 == 1).astype(np.int64)
    fm = np.zeros(N, dtype=np.int64)
    fm[N // 2:] = 1
    out["antipolar"] = fm
    return out


def named_mask(N, name):
    """"random" (K = N/2), "block<seed>" or the name of an edge mask."""
    if name == "random":
        return random_mask(N, N // 2, N + 1)
    if name.startswith("block"):
        return block_mask(N, int(name[5:]))
    return edge_masks(N)[name]


EDGE_NAMES = ("info0", "frozen_last", "K1_mid", "KN-1_mid", "all_info", "alt10", "alt01", "antipolar")
CPU_ALPHABETS = (2, 3, 8, 15, 17, 32, 256)


def cpu_grid(alphabets=CPU_ALPHABETS):
    """The (v, N, mask name, node_rows) cases of the CPU parity tests: every alphabet at N = 16, 64 and 256
    (v = 256 at N = 16 and 32: the tables grow with v^2) with the random mask, a block mask and three of the
    edge masks, taken in turn so that every edge mask meets small and large alphabets; node_rows alternates
    inside each (v, N), so both table layouts meet every alphabet and every mask family.  Ordered so that the
    cases of one table set are adjacent."""
    out, turn = [], 0
    for v in alphabets:
        for N in ((16, 32) if v == 256 else (16, 64, 256)):
            names = ["random", "block%d" % BLOCK_SEEDS.get(N, (3,))[turn % len(BLOCK_SEEDS.get(N, (3,)))]]
            names += [EDGE_NAMES[(turn + 3 * i) % len(EDGE_NAMES)] for i in range(3)]
            for i, name in enumerate(names):
                out.append((v, N, name, (i + turn) % 2 == 1))
            turn += 1
    return out


def ca_frames(crc_encode, fm, A, crc_n, crc_loc, v, B, seed, ebn0=6.0, delta=0.5):
    """B frames that carry a real CRC over the code of mask `fm`, sent over AWGN and quantised to v symbols
    with clip(rint(llr / delta + (v - 1) / 2), 0, v - 1), the quantiser of test_gpu_ca_matches_oracle."""
    fm = np.asarray(fm)
    N, mb = fm.size, np.flatnonzero(fm == 0)
    K = mb.size
    rng = np.random.default_rng(seed)
    msg = rng.integers(0, 2, size=(B, A), dtype=np.uint8)
    u = np.concatenate([msg, crc_encode(msg, crc_n, crc_loc)[:, : K - A]], axis=1)
    x = C.polar_encode(u, mb, N)
    sigma = np.sqrt(1 / (2 * (K / N) * 10 ** (ebn0 / 10)))
    llr = ((1.0 - 2.0 * x) + rng.normal(0, sigma, size=(B, N))) * 2 / sigma ** 2
    return msg, np.clip(np.rint(llr / delta + (v - 1) / 2.0), 0, v - 1).astype(np.int32)


def node_type_of(fm):
    """The node labels the drivers hand to the Fast kinds (codes.identify_nodes) for a frozen mask."""
    fm = np.asarray(fm)
    return C.identify_nodes(fm.size, np.flatnonzero(fm == 0)).astype(np.int32)


def labelled_nodes(fm):
    """[(name, size)] of the labelled nodes of a mask in decoding order (leaves as size 1 R0 / R1)."""
    fm = np.asarray(fm)
    N = fm.size
    nt = node_type_of(fm)
    out = []

    def visit(depth, node):
        t = nt[(1 << depth) + node - 1]
        if t >= 0:
            out.append((NODE_NAMES[int(t)], N >> depth))
            return
        visit(depth + 1, 2 * node)
        visit(depth + 1, 2 * node + 1)

    visit(0, 0)
    return out


def special_root(fm, kind):
    """Whether the Fast kinds refuse the mask: a root labelled R0 / R1 / REP (and SPC for FastSC-LUT)."""
    t = node_type_of(fm)[0]
    if kind == "FastSC-LUT":
        return 0 <= t <= 3
    return kind in ("FastSCL-LUT", "CA-FastSCL-LUT") and 0 <= t <= 2
