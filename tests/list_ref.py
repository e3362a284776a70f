"""All L paths of the SCL-LUT / CA-SCL-LUT restatement (tests/status_ref.py) in the
order qpd_decode_list reports them: the reference's argsort(PML) -- for L <= 8 the
stable argsort -- with every path's K decisions, its metric, its own CRC compare
(the mask of CASCLWithRNTI.cpp:222-224 included) and the candidate that is output.
"""
from __future__ import annotations

import numpy as np

import status_ref


def tail_matches(info, A, crc_n=24, crc_loc=status_ref.CRC24_LOC, mask=None):
    """The CRC compare of one path's K decisions: check-code bits [0, K - A) against info[A:K]."""
    K = len(info)
    cc = status_ref.crc_check_code(info[:A], crc_n, crc_loc)
    if mask is not None and len(mask):
        cc[crc_n - len(mask):] ^= np.asarray(mask, dtype=np.uint8)
    return bool((cc[: K - A] == info[A:K]).all())


def decode(p, frozen, L, symbols, A=None, crc_n=24, crc_loc=status_ref.CRC24_LOC, mask=None):
    """(bits [B, L, K], metric [B, L], passed [B, L] bool or None, chosen [B]) on symbols [B, N]."""
    assert L <= 8, "stable argsort is the reference's sort only up to 16 entries"
    frozen = np.asarray(frozen)
    bits, metric, passed, chosen = [], [], [], []
    for y in np.asarray(symbols):
        info, pml = status_ref._decode_frame(p, frozen, L, y)
        order = np.argsort(pml, kind="stable")
        bits.append(info[order])
        metric.append(pml[order])
        if A is None:
            chosen.append(0)
            continue
        ok = np.array([tail_matches(info[i], A, crc_n, crc_loc, mask) for i in order])
        passed.append(ok)
        chosen.append(int(np.argmax(ok)) if ok.any() else 0)
    return (np.stack(bits).astype(np.uint8), np.stack(metric), np.stack(passed) if A is not None else None,
            np.array(chosen, dtype=np.int32))
