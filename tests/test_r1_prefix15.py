"""The R1 argsort of the fast kernel with up to 15 survivor layers (FastSCL-LUT, L = 9..16;
qpd_fast_special.hpp r1_prep): both of its paths -- the min-tree pick for nodes of <= 16 elements, and
stl::partition_prefix plus the m smallest (rank, position) for 17..32 -- give the first m outputs
of std::sort with a keys-only comparison, m = 1..15, heap-sort fallbacks included."""
import os
import re
import subprocess

from conftest import ROOT


def test_r1_prefix15_matches_std_sort(tmp_path):
    exe = tmp_path / "r1_prefix15_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "quantized_decoder_polar_codes_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "r1_prefix15_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe), "40000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "mismatches=0" in r.stdout
    assert int(re.search(r"heap_fallbacks=(\d+)", r.stdout).group(1)) > 0  # the fallback inputs were not skipped
