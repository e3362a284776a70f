"""csrc/stl_sort.hpp (the device replay of libstdc++ std::sort used for the
FastSCL-LUT R1 argsort, hazard H1) equals std::sort on tie-heavy inputs,
including inputs that drive introsort into its heap-sort fallback."""
import os
import subprocess

from conftest import ROOT


def test_stl_sort_matches_std_sort(tmp_path):
    exe = tmp_path / "stl_sort_check"
    subprocess.run(["g++", "-O2", "-std=c++14", "-I", os.path.join(ROOT, "quantized_decoder_polar_codes_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "stl_sort_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), "60000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mismatches=0" in r.stdout


def test_w16_parallel_replay_matches_std_sort(tmp_path):
    """The W16 kernel's survivor selection for 2L > 16 candidates (qpd_fast_select.hpp
    select_survivors16: dense ranks, the introsort partitions replayed from
    scan-stop masks, the final (rank, position) selection), emulated lane group
    by lane group, gives std::sort's first L outputs (mink, H1) on tie-heavy
    path-metric-like keys, dead (+inf) paths and all-equal lists, L = 9..16.

    A group that reaches the introsort's depth limit replays serially
    (stl::sort_small_prefix on the original keys): those cases are compared with
    std::sort as well, and some must occur -- the deep-partition arrays, the
    adversary arrays, their single-entry mutations and the bounded witness search
    of the checker.  The witnesses it writes are the committed fixture that
    tests/test_gpu_selection.py runs on the device."""
    import json
    import re

    exe = tmp_path / "w16_replay_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "quantized_decoder_polar_codes_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "w16_replay_check.cpp"), "-o", str(exe)], check=True)
    wit = tmp_path / "witnesses.json"
    r = subprocess.run([str(exe), "100000", str(wit)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mismatches=0" in r.stdout
    m = re.search(r"trials=(\d+) mismatches=0 fallbacks=(\d+)", r.stdout)
    assert m and int(m.group(1)) >= 100000 and int(m.group(2)) > 0, r.stdout
    per_l = {int(a): int(b) for a, b in re.findall(r"^L=(\d+) .* fallbacks=(\d+)$", r.stdout, re.M)}
    assert sorted(per_l) == list(range(9, 17)) and per_l[15] > 0, per_l
    # 2L - 2 lg(2L) < 17: no input reaches the depth limit at L <= 12
    assert all(per_l[L] == 0 for L in range(9, 13)), per_l
    with open(wit) as fh, open(os.path.join(ROOT, "tests", "golden", "w16_fallback_witnesses.json")) as gh:
        found, committed = json.load(fh), json.load(gh)
    assert found == committed
    assert all(len(k) == 2 * int(L) for L, ks in committed.items() for k in ks)
    assert {int(L) for L in committed} == {L for L, n in per_l.items() if n > 0}
