"""Every witness of tests/golden/r1_heap_witnesses.json reaches the introsort's depth limit at
the prefix lengths it lists and at no other -- by the script's replay() and by the host
predicate of the R1 harness library (qpd_r1_heap), the two restatements of the partition loop
the GPU test's input conditions rest on.  (The search itself takes about a minute:
`python tests/golden/make_r1_heap_witnesses.py --check` reproduces the file.)"""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, "tests", "golden", "make_r1_heap_witnesses.py")


def _script():
    spec = importlib.util.spec_from_file_location("make_r1_heap_witnesses", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_r1_heap_witnesses_hold():
    mod = _script()
    with open(mod.OUT) as fh:
        text = fh.read()
    doc = json.loads(text)
    assert text == mod.dumps(doc)  # the script's own formatting
    assert len(doc["witnesses"]) >= 3 and {30, 31, 32} <= {w["n"] for w in doc["witnesses"]}
    assert [w["ranks"] for w in doc["witnesses"] if w["from"] == "r1_prefix15_check.cpp"] == sorted(mod.SEEDS, key=lambda r: (len(r), r))
    for w in doc["witnesses"]:
        assert 17 <= w["n"] == len(w["ranks"]) <= 32 and all(0 <= r < 16 for r in w["ranks"])
        assert w["m"] and w["m"] == [m for m in range(1, 16) if mod.replay(w["ranks"], m)[0]]
    sizes = {w["n"] for w in doc["witnesses"]} | {x["n"] for x in doc["none"]}
    assert sizes == set(range(17, 33))  # every size is either witnessed or recorded as having none


def test_r1_heap_predicate_agrees_with_the_script():
    """qpd_r1_heap (host code of the harness library; no device is touched) against replay(): the
    witnesses' m lists and partition counts, and 2000 random and mutated arrays of every size."""
    import random
    import sys

    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import r1_harness

    h = r1_harness.Harness(r1_harness.build())
    mod = _script()
    with open(mod.OUT) as fh:
        wit = json.load(fh)["witnesses"]
    rng = random.Random(3)
    arrays = [w["ranks"] for w in wit]
    for _ in range(2000):
        if rng.randrange(2):
            a = list(rng.choice(wit)["ranks"])
            a[rng.randrange(len(a))] = rng.randrange(16)
        else:
            a = [rng.randrange(1 + rng.randrange(16)) for _ in range(rng.randrange(17, 33))]
        arrays.append(a)
    for a in arrays:
        for m in range(1, 16):
            fell, parts = h.heap(np.array([a]), m)
            want = mod.replay(a, m)
            assert (bool(fell[0]), int(parts[0])) == (want[0], want[1]), (a, m)
    for w in wit:
        assert w["m"] == [m for m in range(1, 16) if h.heap(np.array([w["ranks"]]), m)[0][0]]
