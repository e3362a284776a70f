"""The reference's blind-detection metric restated in numpy, as the tests' checker:
DMetricCalculator::calculate, PolarEncoder/PolarBD/_cpp/src/DMetric.cpp:24-177, with
f / g / u of PolarBD/_cpp/src/utils.cpp:7-24 and sign() of include/utils.h:13.
Written from those files, independently of the library's host engine and kernel
(tests/test_dmetric_ref.py first checks it against the reference's own recorded
doubles, tests/golden/dmetric/dm_*.npz).

The traversal does not depend on the data, so the frames of a batch run side by
side along axis 0; every floating-point operation is the reference's, per frame,
in the reference's order (the node sums are sequential over the elements, :59-61
and :85-87 / :93-95).  Besides the metric it returns the traversal's root ucap
re-encoded to the information bits, which is what the float FastSC decoder returns
for the same walk (FastSCDecoder.cpp:153-172; the calculator itself returns no bits).
"""
import numpy as np


def _sign(x):  # utils.h:13: an int
    return (x > 0).astype(np.int64) - (x < 0).astype(np.int64)


def _f(a, b):  # utils.cpp:9
    return (_sign(a) * _sign(b)).astype(np.float64) * np.minimum(np.abs(a), np.abs(b))


def _g(a, b, u):  # utils.cpp:15
    return (1 - 2 * u.astype(np.int64)).astype(np.float64) * a + b


def _seq_sum(alpha):  # `tmp += palpha[i]` for i = 0 .. temp-1, per frame
    s = np.zeros(alpha.shape[0], dtype=np.float64)
    for i in range(alpha.shape[1]):
        s = s + alpha[:, i]
    return s


def dmetric(N, frozen_bits, node_type, llr):
    """(metric float64 [B], bits uint8 [B, K]) for llr [B, N] (or [N])."""
    frozen = np.asarray(frozen_bits).reshape(-1)
    nt = np.asarray(node_type).reshape(-1)
    llr = np.asarray(llr, dtype=np.float64).reshape(-1, N)
    n = int(np.log2(N))
    assert 1 << n == N and frozen.size == N and nt.size == 2 * N - 1
    B = llr.shape[0]
    acc = [np.zeros(B, dtype=np.float64)]  # DMetric = 0, :36

    def node(depth, idx, alpha):
        """ucap [B, temp] of node `idx` at `depth` from its alpha [B, temp]."""
        temp = N >> depth
        if depth == n:  # :38-45 (a leaf's label is never read)
            if frozen[idx] == 1:
                return np.zeros((B, 1), dtype=np.uint8)
            return (alpha <= 0).astype(np.uint8)
        t = nt[(1 << depth) + idx - 1]
        if t == 0:  # R0, :49-66
            acc[0] = acc[0] + _seq_sum(alpha) / temp  # :57-62
            return np.zeros((B, temp), dtype=np.uint8)
        if t == 1:  # R1, :67-78
            return (alpha <= 0).astype(np.uint8)
        if t == 2:  # REP, :79-101
            S = _seq_sum(alpha)
            acc[0] = acc[0] + np.abs(S) / temp  # :91-97 (the same sum, summed again)
            return np.repeat((S <= 0).astype(np.uint8)[:, None], temp, axis=1)  # :88
        if t == 3:  # SPC, :102-131
            hd = (alpha <= 0).astype(np.uint8)
            odd = hd.sum(axis=1) % 2 == 1
            first_min = np.argmin(np.abs(alpha), axis=1)  # min_element: the first minimum, :120
            rows = np.flatnonzero(odd)
            hd[rows, first_min[rows]] ^= 1
            return hd
        half = temp // 2
        a, b = alpha[:, :half], alpha[:, half:]
        ul = node(depth + 1, 2 * idx, _f(a, b))  # :132-140
        ur = node(depth + 1, 2 * idx + 1, _g(a, b, ul))  # :142-155
        return np.concatenate([ul ^ ur, ur], axis=1)  # u(), :157-166

    x = node(0, 0, llr)
    m = 1
    for _ in range(n):  # FastSCDecoder.cpp:156-164
        x = x.reshape(B, N // (2 * m), 2, m)
        x = np.concatenate([x[:, :, 0] ^ x[:, :, 1], x[:, :, 1]], axis=2).reshape(B, N)
        m *= 2
    return acc[0], np.ascontiguousarray(x[:, frozen == 0])
