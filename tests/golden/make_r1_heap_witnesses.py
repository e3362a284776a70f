#!/usr/bin/env python3
"""Writes tests/golden/r1_heap_witnesses.json: rank arrays of 17..32 entries (ranks < 16,
what an R1 node with its ranks in the op record sorts) on which libstdc++'s introsort
reaches its depth limit -- the heap-sort fallback of partition_prefix_masked
(qpd_fast_special.hpp) -- each with the prefix lengths m at which it does.

The partition loop below restates std::sort's (median of three to the front, Hoare
partition, 2 * floor(lg n) partitions allowed, ranges of <= 16 left to the insertion
sort) with the prefix rule of stl::partition_prefix.  A partition splits off at least
one entry, so the limit needs n - 2 * floor(lg n) > 16: sizes 17..24 have no witness
whatever the keys (recorded under "none").  For the others seeded hill climbs on the
number of partitions start in turn from the three arrays of
tests/native/r1_prefix15_check.cpp, resized, and from random arrays.  Deterministic:
fixed seeds, step and restart counts, no clock (about 20 s).  KNOWN holds witnesses that
longer runs of the same climb found (60000 steps, up to 120 restarts per size); the run
starts from them first, checks them with replay() and so keeps them without repeating
the long search.

usage: python tests/golden/make_r1_heap_witnesses.py [--check]
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "r1_heap_witnesses.json")
THRESHOLD = 16
STEPS = 60000  # hill-climb steps per start
RESTARTS = 6  # starts per size: the resized seeds in turn, every other one a random array

SEEDS = [
    [10, 15, 1, 13, 5, 9, 1, 12, 8, 4, 9, 6, 7, 1, 5, 15, 7, 4, 11, 9, 8, 7, 9, 1, 9, 9, 9, 2, 1, 0, 0],
    [14, 0, 0, 1, 5, 12, 13, 6, 11, 8, 10, 7, 7, 8, 3, 15, 12, 5, 5, 5, 9, 10, 3, 8, 1, 3, 2, 1, 0, 14],
    [0, 14, 0, 13, 1, 9, 5, 15, 8, 5, 4, 4, 8, 6, 12, 3, 5, 8, 3, 4, 9, 4, 4, 2, 1, 12, 12, 0, 10, 13, 13],
]

KNOWN = [  # by longer runs of climb()
    [14, 8, 7, 2, 2, 13, 5, 10, 6, 4, 9, 4, 4, 0, 15, 12, 5, 9, 4, 6, 7, 5, 11, 3, 2, 1, 14, 14, 15],
    [15, 0, 13, 1, 2, 14, 6, 5, 9, 8, 8, 7, 11, 8, 9, 7, 15, 12, 7, 8, 8, 9, 10, 8, 10, 5, 4, 13, 13, 1, 0, 15],
]


def depth_limit(n):
    return 2 * (n.bit_length() - 1)


def replay(rank, m):
    """(reaches the depth limit, partitions run) for the first m outputs of the argsort."""
    e = list(rank)
    n = len(e)
    f, l, dl, end, parts = 0, n, depth_limit(n), n, 0
    while l - f > THRESHOLD:
        if dl == 0:
            return True, parts, l - f
        dl -= 1
        parts += 1
        a, b, c = f + 1, f + (l - f) // 2, l - 1
        if e[a] < e[b]:
            pick = b if e[b] < e[c] else c if e[a] < e[c] else a
        else:
            pick = a if e[a] < e[c] else c if e[b] < e[c] else b
        e[f], e[pick] = e[pick], e[f]
        pv, i, j = e[f], f + 1, l
        while True:
            while e[i] < pv:
                i += 1
            j -= 1
            while pv < e[j]:
                j -= 1
            if not i < j:
                break
            e[i], e[j] = e[j], e[i]
            i += 1
        cut = i
        if cut >= m and cut < end:
            end = cut
        if l - cut > THRESHOLD:
            if cut >= end:
                return False, parts, 0
            f = cut
        else:
            l = cut
    return False, parts, l - f


def ms_of(rank):
    return [m for m in range(1, 16) if replay(rank, m)[0]]


def score(rank):
    """Partitions run at m = 15 (the longest prefix: the most left-stripping partitions count), then
    the entries still in play when the loop stopped; the limit counted on top."""
    fell, parts, left = replay(rank, 15)
    return 64 * parts + left + (10000 if fell else 0)


def resize(seed, n, rng):
    a = list(seed[:n])
    while len(a) < n:
        a.insert(rng.randrange(len(a) + 1), rng.randrange(16))
    return a


def climb(n, start, rng):
    cur, best = list(start), score(start)
    for _ in range(STEPS):
        if best >= 10000:
            break
        cand = list(cur)
        for _ in range(1 + rng.randrange(2)):
            if rng.randrange(4) == 0:
                i, j = rng.randrange(n), rng.randrange(n)
                cand[i], cand[j] = cand[j], cand[i]
            else:
                cand[rng.randrange(n)] = rng.randrange(16)
        sc = score(cand)
        if sc >= best:
            cur, best = cand, sc
    return cur if best >= 10000 else None


def generate():
    doc = {"comment": "rank arrays (ranks < 16) on which std::sort's introsort reaches its depth limit when the "
                      "first m outputs are wanted, per size n; none: sizes without a witness "
                      "(17..24: impossible, n - 2 floor(lg n) <= 16; others: none found by the searches so far)",
           "witnesses": [], "none": []}
    for seed in SEEDS:
        doc["witnesses"].append({"n": len(seed), "ranks": seed, "m": ms_of(seed), "from": "r1_prefix15_check.cpp"})
    have = {len(s) for s in SEEDS}
    for n in range(17, 33):
        if n - depth_limit(n) <= THRESHOLD:
            doc["none"].append({"n": n, "reason": "impossible"})
            continue
        if n in have:
            continue
        found = next((list(a) for a in KNOWN if len(a) == n and replay(a, 15)[0]), None)
        if found:
            doc["witnesses"].append({"n": n, "ranks": found, "m": ms_of(found), "from": "longer search"})
            continue
        for k in range(RESTARTS):
            rng = random.Random(1000 * n + k)
            start = [rng.randrange(16) for _ in range(n)] if k & 1 else resize(SEEDS[(k >> 1) % len(SEEDS)], n, rng)
            found = climb(n, start, rng)
            if found:
                break
        if found:
            doc["witnesses"].append({"n": n, "ranks": found, "m": ms_of(found), "from": "search"})
        else:
            doc["none"].append({"n": n, "reason": "not found"})
    doc["witnesses"].sort(key=lambda w: (w["n"], w["ranks"]))
    return doc


def dumps(doc):
    return json.dumps(doc, indent=1) + "\n"


if __name__ == "__main__":
    text = dumps(generate())
    if "--check" in sys.argv:
        with open(OUT) as fh:
            sys.exit(0 if fh.read() == text else "r1_heap_witnesses.json differs from what the script writes")
    with open(OUT, "w") as fh:
        fh.write(text)
    print(f"wrote {OUT}")
