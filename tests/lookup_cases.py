"""Inputs of the lookup harness tests, built in numpy, with the expected results from
tests/lookup_ref.py.  The generators assert their own coverage: every cell of the stated
domain -- (element position, index a * 16 + b, table half) for the lookups, (position, value)
for the channel readers -- is carried by at least one lane, or the generator raises.
tests/test_lookup_cases.py runs them without a GPU; tests/test_gpu_lookup.py feeds them to
the device.

Don't-care bits are filled with random garbage where the product's callers pass garbage:
  lut_vec<2|4>   nibbles >= NE of A and B (callers pass W, W >> 8 / W >> 16) and the bits >= NE of hi (the
                 whole u word of the op)
  lut_vec<8>, lut_lds<8, g>   the bits >= 8 of hi (fg_op passes ub >> (k << 3), the next words' u bits above)
  lut_byte       the bytes >= NE of W (BOT3 passes x[s][1]: c3 << 27 and the leaf fields above) and the bits
                 of H outside 8 k + 7
  nib_mask       the bits >= 8 (gsel_op passes u >> ((k & 3) << 3))
The f forms get hi = 0, as every caller passes it (ub = 0 for f: entries below 256).
"""
import numpy as np

import lookup_ref as R

LOOKUP_V = [2, 3, 15, 16]
CHAN_V = [2, 3, 8, 15, 16]
I32_EXTRA = [-1, 2 ** 31 - 1, -2 ** 31, 0x7FFF0000, -65536]  # beside 0..255 (16 among them); the last two: only high bits set


# -- tables -------------------------------------------------------------------------------------
def _spread(rng, m):
    """m nibbles: every value 0..15 present (m >= 16), or all distinct (m < 16)."""
    x = np.concatenate([rng.permutation(16) for _ in range(m // 16 + 1)])[:m]
    if m > 16:
        x[16:] = rng.integers(0, 16, size=m - 16)
    return rng.permutation(x).astype(np.uint8)


def random_tables(v, rng):
    """tf [2, v, v] (the op's f table and the folded child's), tg [2, v, v] (u = 0, u = 1)."""
    return _spread(rng, 2 * v * v).reshape(2, v, v), _spread(rng, 2 * v * v).reshape(2, v, v)


def closed_tables(v, rng):
    """Tables whose entries are symbols of the alphabet again (< v), as a decoder's are: for the ops that
    feed one lookup's results to the next (ff_op)."""
    tf, tg = random_tables(v, rng)
    return tf % v, tg % v


def index_tables(v):
    """T[i] = i & 15 (= b) and T[i] = i >> 4 (= a), i = a * 16 + b: a swapped a / b or a shifted index
    cannot hide behind a symmetric table.  tf = [b, a]; tg = [u = 0: b, u = 1: a]."""
    a, b = np.meshgrid(np.arange(v), np.arange(v), indexing="ij")
    t = np.stack([b, a]).astype(np.uint8)
    return t.copy(), t.copy()


def table_sets(v, seed):
    return {"random": random_tables(v, np.random.default_rng(seed)), "index": index_tables(v)}


# -- lookups ------------------------------------------------------------------------------------
def lookup_elements(ne, v, halves, rng):
    """Per lane the ne elements (a, b, u): lane (k, a, b, u) carries exactly that combination in element k,
    the other elements random.  Returns a, b, u as [lanes, ne]."""
    k, a, b, u = [x.reshape(-1) for x in np.meshgrid(np.arange(ne), np.arange(v), np.arange(v), np.arange(halves), indexing="ij")]
    n = k.size
    A = rng.integers(0, v, size=(n, ne))
    Bm = rng.integers(0, v, size=(n, ne))
    U = rng.integers(0, halves, size=(n, ne))
    rows = np.arange(n)
    A[rows, k], Bm[rows, k], U[rows, k] = a, b, u
    return A, Bm, U


def assert_lookup_coverage(a, b, u, ne, v, halves):
    """Every (k, a * 16 + b, half) cell is hit: 100 % or an AssertionError."""
    hit = np.zeros((ne, 256, halves), bool)
    for k in range(ne):
        hit[k, a[:, k] * 16 + b[:, k], u[:, k]] = True
    want = np.zeros(256, bool)
    want[(np.arange(v)[:, None] * 16 + np.arange(v)[None, :]).reshape(-1)] = True
    cov = hit[:, want, :]
    assert cov.all(), f"lookup coverage {cov.mean():.4f} of ne={ne} v={v} halves={halves}"
    return float(cov.mean())


def _garbage(rng, n, mask):
    return rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32) & np.uint32(mask)


def _bits_word(u):
    return R.word_of(u)


def vec_case(ne, v, isg, il, rng):
    """lut_vec<ne[, il]> / lut_lds<8, isg, ., il>: operands (A, B, hi) and the elements they carry."""
    halves = 2 if isg else 1
    a, b, u = lookup_elements(ne, v, halves, rng)
    n = a.shape[0]
    low = (1 << (4 * ne)) - 1
    A = R.pack_word(a) | _garbage(rng, n, ~low & 0xFFFFFFFF)
    B = R.pack_word(b) | _garbage(rng, n, ~low & 0xFFFFFFFF)
    hi = (_bits_word(u) | _garbage(rng, n, ~((1 << ne) - 1) & 0xFFFFFFFF)) if isg else np.zeros(n, np.uint32)
    # coverage from the operand words themselves, as the device reads them
    ua = R.unpack_words(A[:, None])[:, :ne].astype(np.int64)
    ub = R.unpack_words(B[:, None])[:, :ne].astype(np.int64)
    uu = R.bits_of(hi)[:, :ne].astype(np.int64)
    cov = assert_lookup_coverage(ua, ub, uu, ne, v, halves)
    return dict(A=A, B=B, H=hi, a=a, b=b, u=u, ne=ne, il=il, isg=isg, coverage=cov)


def byte_case(ne, v, has_h, il, rng):
    """lut_byte<ne, il, has_h>: W in interleaved order (byte k = a_k * 16 + b_k), H bit 8 k + 7 = half of k."""
    halves = 2 if has_h else 1
    a, b, u = lookup_elements(ne, v, halves, rng)
    n = a.shape[0]
    W = np.zeros(n, np.uint32)
    H = np.zeros(n, np.uint32)
    hmask = 0
    for k in range(ne):
        W |= ((a[:, k] * 16 + b[:, k]).astype(np.uint32)) << np.uint32(8 * k)
        H |= u[:, k].astype(np.uint32) << np.uint32(8 * k + 7)
        hmask |= 1 << (8 * k + 7)
    W |= _garbage(rng, n, ~((1 << (8 * ne)) - 1) & 0xFFFFFFFF)
    H = (H | _garbage(rng, n, ~hmask & 0xFFFFFFFF)) if has_h else np.zeros(n, np.uint32)
    wb = np.stack([(W >> np.uint32(8 * k)) & np.uint32(255) for k in range(ne)], axis=1).astype(np.int64)
    hb = np.stack([(H >> np.uint32(8 * k + 7)) & np.uint32(1) for k in range(ne)], axis=1).astype(np.int64)
    cov = assert_lookup_coverage(wb >> 4, wb & 15, hb, ne, v, halves)
    return dict(A=W, B=np.zeros(n, np.uint32), H=H, a=a, b=b, u=u, ne=ne, il=il, isg=has_h, coverage=cov)


def lut4_case(v, rng):
    a, b, u = lookup_elements(1, v, 2, rng)
    idx = (u[:, 0] * 256 + a[:, 0] * 16 + b[:, 0]).astype(np.uint32)
    cov = assert_lookup_coverage((idx[:, None] >> 4) & 15, idx[:, None] & 15, idx[:, None] >> 8, 1, v, 2)
    return dict(A=np.zeros(idx.size, np.uint32), B=idx, H=np.zeros(idx.size, np.uint32), a=a, b=b, u=u, ne=1, il=False, isg=True,
                coverage=cov)


def lookup_expected(case, tf, tg, v):
    """The result word: f (the op's table) or g of every element, element k at nibble k or in interleaved order."""
    if case["isg"]:
        out = R.g_elem(tg, v, case["u"], case["a"], case["b"])
    else:
        out = R.f_elem(tf, v, case["a"], case["b"])
    return R.pack_il(out) if case["il"] else R.pack_word(out)


# -- helpers ------------------------------------------------------------------------------------
def helper_cases(rng):
    """name -> (input words, expected words), every one over its stated domain."""
    out = {}
    all16 = np.arange(1 << 16, dtype=np.uint32)
    nib4 = R.unpack_words(all16[:, None])[:, :4].astype(np.uint32)  # the four nibbles of every 16-bit word
    spread = nib4[:, 0] | (nib4[:, 1] << 8) | (nib4[:, 2] << 16) | (nib4[:, 3] << 24)
    out["nib_pack4"] = (spread, all16)   # bytes 0-3 (each < 16) -> nibbles 0-3: all 2^16
    out["nib2byte4"] = (all16, spread)   # and back
    c2, c4 = np.arange(4, dtype=np.uint32), np.arange(16, dtype=np.uint32)
    out["half_bits2"] = (c2, sum(((c2 >> k) & 1) << (8 * k + 7) for k in range(2)).astype(np.uint32))
    out["half_bits4"] = (c4, sum(((c4 >> k) & 1) << (8 * k + 7) for k in range(4)).astype(np.uint32))
    b8 = np.tile(np.arange(256, dtype=np.uint32), 4)
    b8 = b8 | _garbage(rng, b8.size, 0xFFFFFF00)
    b8[:256] &= 255
    out["nib_mask"] = (b8, R.pack_word(R.bits_of(b8)[:, :8] * 15))
    k8 = np.arange(8, dtype=np.uint32)
    pos = [np.array(R.il_positions(ne), np.uint32) for ne in (8, 4, 2)]
    out["il_nib"] = (k8, pos[0][k8 & 7] | (pos[1][k8 & 3] << 8) | (pos[2][k8 & 1] << 16))
    walk = np.array([val << (4 * p) for p in range(8) for val in range(1, 16)], np.uint32)
    wi = np.concatenate([walk, _garbage(rng, 4096, 0xFFFFFFFF)])
    out["nib_interleave8"] = (wi, R.pack_il(R.unpack_words(wi[:, None])))
    pw = np.concatenate([np.uint32(1) << np.arange(32, dtype=np.uint32), _garbage(rng, 4096, 0xFFFFFFFF)])
    out["polar_word"] = (pw, R.polar_word(pw))
    # the generators' own coverage
    assert np.array_equal(np.unique(out["nib_pack4"][1]), all16) and np.array_equal(np.unique(out["nib2byte4"][0]), all16)
    assert set(b8 & 255) == set(range(256)) and walk.size == 120 and len(set(walk.tolist())) == 120
    return out


# -- channel readers ------------------------------------------------------------------------------
def chan_case(u8, v, base, rng, counted=False):
    """One 8-symbol group per lane: lane (pos, value) holds `value` at position pos, the rest valid.  The
    groups lie one after the other from element `base` on.  counted: a count 0..8 per lane (chan_word,
    chan_small); every (pos, value) cell also appears with a count that includes it.
    Returns buf, e0, cnt, and the expected (word, error word) per lane."""
    vals = list(range(256)) + ([] if u8 else I32_EXTRA)
    pos, val = [x.reshape(-1) for x in np.meshgrid(np.arange(8), np.array(vals, np.int64), indexing="ij")]
    reps = 2 if counted else 1
    pos, val = np.tile(pos, reps), np.tile(val, reps)
    n = pos.size
    pad = (-n) % 64
    pos, val = np.concatenate([pos, pos[:pad]]), np.concatenate([val, val[:pad]])
    n += pad
    sym = rng.integers(0, v, size=(n, 8)).astype(np.int64)
    sym[np.arange(n), pos] = val
    cnt = np.full(n, 8, np.int64)
    if counted:
        half = n // 2
        cnt[:half] = rng.integers(pos[:half] + 1, 9)  # the cell inside the count
        cnt[half:] = rng.integers(0, 9, size=n - half)  # any count: a bad symbol past it must not show
    buf = np.concatenate([rng.integers(0, v, size=base), sym.reshape(-1)])
    buf = buf.astype(np.uint8) if u8 else buf.astype(np.int64).astype(np.int32)
    e0 = base + 8 * np.arange(n)
    clean, bad = R.clean_channel(sym, v)
    inside = np.arange(8)[None, :] < cnt[:, None]
    word = R.pack_word(np.where(inside, clean, 0))
    err = (bad & inside).any(axis=1).astype(np.int32)
    hit = np.zeros((8, len(vals)), bool)
    index = {x: i for i, x in enumerate(vals)}
    for p, x, c in zip(pos, val, cnt):
        if p < c:
            hit[p, index[int(x)]] = True
    assert hit.all(), f"channel coverage {hit.mean():.4f} (u8={u8}, v={v})"
    return dict(buf=buf, e0=e0.astype(np.int32), cnt=cnt.astype(np.int32), word=word, err=err, coverage=float(hit.mean()))


# -- ops ------------------------------------------------------------------------------------------
PAD_WORD = 0x5A5A0000


def _perm_fields(rng, nb, ns, gs):
    """A non-identity permutation inside each lane group (gs >= 2): [nb, ns, 64] slots."""
    out = np.zeros((nb, ns, 64), np.uint8)
    for b in range(nb):
        for s in range(ns):
            for g in range(0, 64, gs):
                p = rng.permutation(gs)
                if gs > 1 and (p == np.arange(gs)).all():
                    p = np.roll(p, 1)
                out[b, s, g:g + gs] = p
    return out


def _u_bits(rng, shape, nbits):
    """u bits [..., nbits] whose bytes are distinct within every 32-bit word (a wrong byte shift shows)."""
    nwords = max(1, -(-nbits // 32))
    order = np.argsort(rng.random(shape + (nwords, 256)), axis=-1)[..., :4]  # 4 distinct bytes per word
    by = order.reshape(shape + (4 * nwords,)).astype(np.uint8)
    return np.unpackbits(by, axis=-1, bitorder="little")  # [..., 32 * nwords] (bits past nbits: garbage)


def op_case(kind, isg, cnt, v, ns, gs, spaces, tf, tg, rng, nb=3, pre=False, in_vec=False, bad_symbols=False):
    """One op on rows the test chose.  kind: "fg", "fgp" (fg_op<., false>), "chan", "ff", "gsel".
    spaces: bit 0 S[d] in LDS, 1 destination in LDS, 2 U rows in LDS, 3 (ff) S[d + 2] in LDS.
    Returns the harness arguments and the expected LDS / slab images and error words."""
    sl, dl, ul, cdl = bool(spaces & 1), bool(spaces & 2), bool(spaces & 4), bool(spaces & 8)
    nwo = cnt // 8 if cnt >= 8 else 1
    nwc = nwo // 2
    nsrcw = 2 * nwo if cnt >= 8 else 1
    nuw = -(-nwo // 4)
    rowsrc = kind in ("fg", "ff") or (kind == "fgp" and not pre)
    # rows of each space one region after the other, a pad row before, between and after them
    nxt = {True: 1, False: 1}

    def place(in_lds, n):
        at = nxt[in_lds]
        nxt[in_lds] = at + n + 1
        return at

    src_row = place(sl, nsrcw) if rowsrc else 0
    dst_row = place(dl, nwo)
    u_row = place(ul, nuw) if isg else 0
    r_row = place(cdl, nwc) if kind == "ff" else 0
    lds_rows, glb_rows = nxt[True], nxt[False]

    def pattern(rows):
        r, s, l = np.meshgrid(np.arange(rows), np.arange(ns), np.arange(64), indexing="ij")
        img = (PAD_WORD | (r << 8) | (s << 7) | l).astype(np.uint32)
        return np.stack([img ^ np.uint32(b * 0x01010101) for b in range(nb)])

    img = {True: pattern(lds_rows), False: pattern(glb_rows)}
    srcf, usrcf = _perm_fields(rng, nb, ns, gs), _perm_fields(rng, nb, ns, gs)
    lanes = np.arange(64)
    src = (lanes - lanes % gs)[None, None, :] + srcf  # the column lane l reads
    usrc = (lanes - lanes % gs)[None, None, :] + usrcf
    fpg = 64 // gs
    take = lambda x, col: np.take_along_axis(x, col[..., None].astype(np.int64), axis=2)  # noqa: E731
    # u bits per column (the U rows' lane), garbage above cnt
    ubits = _u_bits(rng, (nb, ns, 64), cnt)
    uw = R.word_of(ubits.reshape(nb, ns, 64, nuw, 32))  # [nb, ns, 64, words]: bit j of u in word j // 32
    if isg:
        for w in range(nuw):
            img[ul][:, u_row + w] = uw[..., w]
    u_lane = take(ubits, usrc)[..., :cnt].astype(np.int64)  # the bits lane l sees
    err = np.zeros(nb, np.int32)
    ystride = 4
    y = np.zeros((nb, ns, fpg, ystride), np.int32)
    if rowsrc:  # S[d] per column
        sym = rng.integers(0, v, size=(nb, ns, 64, 2 * cnt))
        words = R.pack_words(sym) if cnt >= 8 else R.pack_word(sym)[..., None]
        for w in range(nsrcw):
            img[sl][:, src_row + w] = words[..., w]
        node = take(sym, src)
    elif kind == "chan":
        ystride = 2 * cnt + (4 if in_vec else 3)  # in_vec: the rows stay 16-byte aligned
        ystride += (-ystride) % 4 if in_vec else 0
        ysym = rng.integers(0, v, size=(nb, ns, fpg, ystride)).astype(np.int64)
        if bad_symbols:  # out-of-range symbols in one block's frames, the others clean
            for (s, f, e, val) in [(0, 0, 0, v), (ns - 1, fpg - 1, 2 * cnt - 1, -1), (0, fpg // 2, cnt, 255)]:
                ysym[1, s, f, e] = val
            ysym[2, 0, 0, 2 * cnt] = 99  # past the root: not read
            err[1] = 1
        y = ysym.astype(np.int32)
        clean, _ = R.clean_channel(ysym[..., :2 * cnt], v)
        node = np.repeat(clean, gs, axis=2)  # every lane of a frame's group reads the frame
    else:  # pre-pass rows: whole words from y
        nodes = rng.integers(0, 16 if kind == "gsel" else v, size=(nb, ns, fpg, 2 * cnt))
        src_row = 3  # the words lie at src_row of the frame's row
        ystride = src_row + 2 * nwo + 2
        yw = _garbage(rng, nb * ns * fpg * ystride, 0xFFFFFFFF).reshape(nb, ns, fpg, ystride)
        yw[..., src_row:src_row + 2 * nwo] = R.pack_words(nodes)
        y = yw.view(np.int32)
        node = np.repeat(nodes, gs, axis=2)
    # the op, from its definition
    if kind == "gsel":
        out = R.nibble_select(node[..., :cnt], node[..., cnt:], u_lane)
    elif isg:
        out = R.g_node(tg, v, node, u_lane)
    else:
        out = R.f_node(tf[0], v, node)
    exp = {True: img[True].copy(), False: img[False].copy()}
    ow = R.pack_words(out) if cnt >= 8 else R.pack_word(out)[..., None]
    for w in range(nwo):
        exp[dl][:, dst_row + w] = ow[..., w]
    if kind == "ff":
        cw = R.pack_words(R.f_node(tf[1], v, out.astype(np.int64)))
        for w in range(nwc):
            exp[cdl][:, r_row + w] = cw[..., w]
    return dict(kind=kind, isg=isg, pre=pre, cnt=cnt, v=v, in_vec=in_vec, gs=gs, spaces=spaces,
                rows=np.array([src_row, dst_row, u_row, r_row], np.int32), y=y, lds=img[True], slab=img[False],
                srcf=srcf, usrcf=usrcf, exp_lds=exp[True], exp_slab=exp[False], exp_err=err,
                nonidentity=bool(gs == 1 or ((srcf != (lanes % gs)).any() and (srcf != usrcf).any())))


# -- root pre-pass ----------------------------------------------------------------------------------
SENTINEL = 0xDEADBEEF


def root_pre_case(u8, n, B, v, in_off, tf, tg, rng, bad_symbols=False):
    N = 1 << n
    y = rng.integers(0, v, size=(B, N)).astype(np.int64)
    err = 0
    if bad_symbols:
        y[0, 0], y[B // 2, N - 1], y[B - 1, N // 2] = v, 255, 16
        err = 1
    clean, _ = R.clean_channel(y, v)
    row = R.pack_words(R.pre_row(tf[0], tg, v, clean))  # [B, 3 N / 16]
    pre = np.full((B + 1, N // 4), SENTINEL, np.uint32)
    exp = pre.copy()
    exp[:B, :3 * N // 16] = row
    lead = rng.integers(0, v, size=in_off)
    inp = np.concatenate([lead, y.reshape(-1)])
    inp = inp.astype(np.uint8) if u8 else inp.astype(np.int32)
    return dict(inp=inp, pre=pre.reshape(-1), exp=exp.reshape(-1), err=err)
