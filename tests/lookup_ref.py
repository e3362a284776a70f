"""Plain numpy reference of the fast engine's table lookups and f / g ops.

Every function is written from the operation's definition on unpacked symbol arrays (one
symbol per array element): no SWAR, no packing tricks, nothing imported from the device
harness or from csrc/.  tests/test_lookup_cases.py pins f and g to the reference decoder
(an SC-LUT decode built from them alone must give the oracle's bits); tests/test_gpu_lookup.py
compares the device functions with them.

Tables are raw: tf[a * v + b] (uint8 [v, v]) and tg[u * v * v + a * v + b] (uint8 [2, v, v]).
"""
import numpy as np


# -- the operations -----------------------------------------------------------------------
def f_elem(tf, v, a, b):
    """out[i] = tf[a[i] * v + b[i]]"""
    return np.asarray(tf, np.uint8).reshape(-1)[np.asarray(a, np.int64) * v + np.asarray(b, np.int64)]


def g_elem(tg, v, u, a, b):
    """out[i] = tg[u[i] * v * v + a[i] * v + b[i]]"""
    idx = np.asarray(u, np.int64) * v * v + np.asarray(a, np.int64) * v + np.asarray(b, np.int64)
    return np.asarray(tg, np.uint8).reshape(-1)[idx]


def f_node(tf, v, sym):
    """f of a node: sym [..., 2h] -> [..., h], a the first half of the node and b the second."""
    h = sym.shape[-1] // 2
    return f_elem(tf, v, sym[..., :h], sym[..., h:])


def g_node(tg, v, sym, u):
    """g of a node: sym [..., 2h], u [..., h] (the left child's partial sums) -> [..., h]."""
    h = sym.shape[-1] // 2
    return g_elem(tg, v, u, sym[..., :h], sym[..., h:])


def pre_row(tf, tg, v, y):
    """The root pre-pass row of channel symbols y [..., N]: [f(y) | g(y, 0) | g(y, 1)], N / 2 symbols each."""
    h = y.shape[-1] // 2
    zero = np.zeros(y.shape[:-1] + (h,), np.int64)
    return np.concatenate([f_node(tf, v, y), g_node(tg, v, y, zero), g_node(tg, v, y, zero + 1)], axis=-1)


def clean_channel(y, v):
    """Channel symbols as the readers see them: an out-of-range symbol reads as 0.  Returns the
    symbols and, per symbol, whether it was out of range."""
    y = np.asarray(y).astype(np.int64)
    bad = (y < 0) | (y >= v)
    return np.where(bad, 0, y), bad


# -- words --------------------------------------------------------------------------------
def pack_words(sym):
    """[..., 8 k] symbols (< 16) -> [..., k] uint32 words, symbol j in nibble j % 8 of word j // 8."""
    sym = np.asarray(sym)
    assert sym.shape[-1] % 8 == 0
    s = sym.reshape(sym.shape[:-1] + (sym.shape[-1] // 8, 8)).astype(np.uint32)
    out = np.zeros(s.shape[:-1], np.uint32)
    for i in range(8):
        out |= s[..., i] << np.uint32(4 * i)
    return out


def pack_word(sym):
    """[..., m] symbols, m <= 8 -> one uint32 word each, symbol j in nibble j."""
    sym = np.asarray(sym).astype(np.uint32)
    out = np.zeros(sym.shape[:-1], np.uint32)
    for i in range(sym.shape[-1]):
        out |= sym[..., i] << np.uint32(4 * i)
    return out


def unpack_words(words, per_word=8):
    """[..., k] words -> [..., k * per_word] symbols (the low per_word nibbles of each word)."""
    w = np.asarray(words, np.uint32)
    out = np.stack([(w >> np.uint32(4 * i)) & np.uint32(15) for i in range(per_word)], axis=-1)
    return out.reshape(w.shape[:-1] + (w.shape[-1] * per_word,)).astype(np.uint8)


def il_positions(ne):
    """The interleaved order of a word of ne symbols: element k (k < ne / 2) in the high nibble of byte
    k, element k + ne / 2 in the low nibble of byte k.  Returns the nibble of every element."""
    pos = []
    for k in range(ne):
        byte, high = (k, 1) if k < ne // 2 else (k - ne // 2, 0)
        pos.append(2 * byte + high)
    return pos


def pack_il(sym):
    """[..., ne] symbols -> one word each in interleaved order."""
    sym = np.asarray(sym).astype(np.uint32)
    out = np.zeros(sym.shape[:-1], np.uint32)
    for k, p in enumerate(il_positions(sym.shape[-1])):
        out |= sym[..., k] << np.uint32(4 * p)
    return out


def unpack_il(words, ne):
    w = np.asarray(words, np.uint32)
    return np.stack([(w >> np.uint32(4 * p)) & np.uint32(15) for p in il_positions(ne)], axis=-1).astype(np.uint8)


def bits_of(x, nbits=32):
    x = np.asarray(x, np.uint64)
    return np.stack([(x >> np.uint64(i)) & np.uint64(1) for i in range(nbits)], axis=-1).astype(np.uint8)


def word_of(bits):
    bits = np.asarray(bits).astype(np.uint64)
    out = np.zeros(bits.shape[:-1], np.uint64)
    for i in range(bits.shape[-1]):
        out |= bits[..., i] << np.uint64(i)
    return out.astype(np.uint32)


def polar_matrix(m=5):
    """F^{(x) m}, F = [[1, 0], [1, 1]]."""
    F = np.array([[1, 0], [1, 1]], np.int64)
    M = np.array([[1]], np.int64)
    for _ in range(m):
        M = np.kron(M, F)
    return M


def polar_word(x):
    """The word x as a row vector of 32 bits (bit i = component i) times F^{(x) 5} over GF(2)."""
    return word_of((bits_of(x).astype(np.int64) @ polar_matrix(5)) % 2)


def nibble_select(g0, g1, u):
    """Symbols g0 / g1 [..., m] chosen per element by the bits u [..., m]."""
    return np.where(np.asarray(u).astype(bool), g1, g0)


# -- the CPU pin: SC-LUT from f and g alone -----------------------------------------------------
def sc_lut_decode(packed, frozen, symbols):
    """SC-LUT on symbols [B, N] (one table per node): f / g by f_node / g_node, the leaf decision
    virtual_channel_llr[n - 1][k][s] <= 0 on the depth n - 1 node's f / g symbol (frozen leaves 0),
    combine [l ^ r, r]; output = the decisions at the information positions."""
    N, v = packed.N, packed.v
    n = N.bit_length() - 1
    assert packed.f_step == 0 and packed.g_step == 0
    frozen = np.asarray(frozen)
    sym = np.asarray(symbols).astype(np.int64)
    B = sym.shape[0]
    bits = np.zeros((B, N), np.uint8)

    def leaf(k, s):
        if frozen[k] != 1:
            bits[:, k] = packed.vcl[n - 1, k, s[:, 0]] <= 0
        return bits[:, k:k + 1].copy()

    def visit(d, node, s):
        posi = (1 << d) + node - 1
        tf, tg = packed.lut_f[packed.f_base[posi]], packed.lut_g[packed.g_base[posi]]
        lo = f_node(tf, v, s).astype(np.int64)
        ul = visit(d + 1, 2 * node, lo) if d + 1 < n else leaf(2 * node, lo)
        hi = g_node(tg, v, s, ul).astype(np.int64)
        ur = visit(d + 1, 2 * node + 1, hi) if d + 1 < n else leaf(2 * node + 1, hi)
        return np.concatenate([ul ^ ur, ur], axis=1)

    visit(0, 0, sym)
    return bits[:, frozen == 0]
