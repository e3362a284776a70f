"""Plain-numpy restatement of the reference's SCL-LUT and CA-SCL-LUT decoders
(SCLLUTDecoder.cpp:47-253, CASCLLUTDecoder.cpp:263-290) that keeps what they
drop: the final path metrics and the CRC verdict, with the CRC mask of
CASCLWithRNTI.cpp:222-224.  For L <= 8: mink / argsort sort at most 16 entries,
where libstdc++'s std::sort is an insertion sort, i.e. numpy's stable argsort.

Same walk as the reference (node_state 0 -> f, 1 -> g, 2 -> combine), same
per-path arrays (symbols / ucap [L][(n + 1) N]) and whole-path copies at a fork;
tables in the packed layout of quantized_decoder_polar_codes_amd/lut.py.
tests/test_status_host.py checks it against the reference's own fixtures before
anything is compared with it.
"""
from __future__ import annotations

import numpy as np

CRC24_LOC = (24, 23, 21, 20, 17, 15, 13, 12, 8, 4, 2, 1, 0)


def crc_check_code(info, crc_n=24, crc_loc=CRC24_LOC):
    """CRC::encoding (utils.cpp:77-92): the crc_n check bits of `info`."""
    p = np.zeros(crc_n + 1, dtype=np.uint8)
    p[list(crc_loc)] = 1
    u = np.concatenate([np.asarray(info, dtype=np.uint8), np.zeros(crc_n, dtype=np.uint8)])
    for i in range(len(info)):
        if u[i]:
            u[i:i + crc_n + 1] ^= p
    return u[len(info):]


def _decode_frame(p, frozen, L, y):
    N, v = p.N, p.v
    n = N.bit_length() - 1
    lut_f = p.lut_f.reshape(-1, v, v)
    lut_g = p.lut_g.reshape(-1, 2, v, v)
    vcl = p.vcl.reshape(-1, N, v)
    sym = np.zeros((L, n + 1, N), dtype=np.int64)
    sym[:, 0, :] = y
    ucap = np.zeros((L, n + 1, N), dtype=np.uint8)
    pml = np.full(L, np.inf)  # DOUBLE_INF of SCLLUTDecoder.h: 1.0 / 0.0
    pml[0] = 0.0
    state = np.zeros(2 * N - 1, dtype=np.int8)
    rows = np.arange(L)

    def leaf(pos, dm):
        nonlocal sym, ucap, pml
        if frozen[pos] == 1:
            ucap[:, n, pos] = 0
            pml = pml + np.abs(dm) * (dm < 0)
            return
        decision = (dm < 0).astype(np.uint8)
        pm2 = np.concatenate([pml, pml + np.abs(dm)])
        posi = np.argsort(pm2, kind="stable")[:L]  # mink: std::sort of 2L <= 16 entries
        pml = pm2[posi]
        upper = posi >= L
        src = np.where(upper, posi - L, posi)
        decision = decision[src] ^ upper.astype(np.uint8)
        sym = sym[src].copy()
        ucap = ucap[src].copy()
        ucap[:, n, pos] = decision

    depth = node = 0
    while True:
        if depth == n:
            if node == N - 1:
                break
            node //= 2
            depth -= 1
            continue
        posi = (1 << depth) + node - 1
        temp = 1 << (n - depth)
        ct = temp // 2
        a = sym[:, depth, temp * node: temp * node + ct]
        b = sym[:, depth, temp * node + ct: temp * node + temp]
        j = np.arange(ct)
        if state[posi] == 0:
            t = p.f_base[posi] + j * p.f_step
            s = lut_f[t[None, :], a, b]
            if depth + 1 < n:
                sym[:, depth + 1, ct * 2 * node: ct * 2 * node + ct] = s
            else:
                leaf(2 * node, vcl[n - 1, 2 * node, s[:, 0]])
            state[posi] = 1
            node, depth = 2 * node, depth + 1
        elif state[posi] == 1:
            ul = ucap[:, depth + 1, 2 * node * ct: 2 * node * ct + ct].astype(np.int64)
            t = p.g_base[posi] + j * p.g_step
            s = lut_g[t[None, :], ul, a, b]
            if depth + 1 < n:
                sym[:, depth + 1, ct * (2 * node + 1): ct * (2 * node + 1) + ct] = s
            else:
                leaf(2 * node + 1, vcl[n - 1, 2 * node + 1, s[:, 0]])
            state[posi] = 2
            node, depth = 2 * node + 1, depth + 1
        else:
            ul = ucap[:, depth + 1, 2 * node * ct: 2 * node * ct + ct]
            ur = ucap[:, depth + 1, (2 * node + 1) * ct: (2 * node + 1) * ct + ct]
            ucap[:, depth, temp * node: temp * node + ct] = ul ^ ur
            ucap[:, depth, temp * node + ct: temp * node + temp] = ur
            state[posi] = 3
            node, depth = node // 2, depth - 1
    del rows
    return ucap[:, n, :][:, np.asarray(frozen) == 0], pml


def select(walked, A=None, crc_n=24, crc_loc=CRC24_LOC, mask=None):
    """The output stage on walked frames [(info [L, K], pml [L])]: SCL-LUT's first minimum (A None) or
    CA-SCL-LUT's CRC walk in argsort(pml) order.  Returns (bits, pml, winner, passed) as decode."""
    out, pmls, winners, passed = [], [], [], []
    for info, pml in walked:
        if A is None:
            w, ok = int(np.argmin(pml)), False  # argmin: the first minimum
            bits = info[w]
        else:
            K = info.shape[1]
            order = np.argsort(pml, kind="stable")
            w, ok = int(order[0]), False
            for i in order:
                cc = crc_check_code(info[i, :A], crc_n, crc_loc)
                if mask is not None and len(mask):
                    cc[crc_n - len(mask):] ^= np.asarray(mask, dtype=np.uint8)
                if (cc[: K - A] == info[i, A:K]).all():
                    w, ok = int(i), True
                    break
            bits = info[w, :A]
        out.append(bits)
        pmls.append(pml)
        winners.append(w)
        passed.append(ok)
    return np.stack(out).astype(np.uint8), np.stack(pmls), np.array(winners), np.array(passed, dtype=bool)


def decode(p, frozen, L, symbols, A=None, crc_n=24, crc_loc=CRC24_LOC, mask=None):
    """SCL-LUT (A None) or CA-SCL-LUT on symbols [B, N] with the packed tables `p`.
    Returns (bits [B, K or A], pml [B, L] final path metrics, winner [B] path index,
    passed [B] bool).  `mask`: 0/1 entries XORed onto the tail of the check code."""
    assert L <= 8, "stable argsort is the reference's sort only up to 16 entries"
    frozen = np.asarray(frozen)
    return select([_decode_frame(p, frozen, L, y) for y in np.asarray(symbols)], A, crc_n, crc_loc, mask)
