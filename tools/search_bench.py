#!/usr/bin/env python3
"""Mask search against its alternatives, and the existing decode calls against another build.

    tools/search_bench.py search [--frames N] [--rounds R]            -> JSON lines
    tools/search_bench.py ab --other PATH/libqpd.so [--frames N] [--rounds R]

Workload: bench.py's CA-SCL-LUT N = 1024, A = 488, K = 512, L = 8 on the min-sum tables, resident uint8
symbols of Monte-Carlo frames at 2 dB.  Times are kernel times (qpd_profile: HIP events around every
launch of the call, all kernel classes summed), the median [min, max] over the rounds.

search: one qpd_decode_search over 8 masks, 8 qpd_decode_status calls (one per mask), one
qpd_decode_list call, one plain qpd_decode_u8 -- alternating within each round.  The HBM bytes of each
tail per frame are arithmetic from the outputs' sizes (include/qpd.h), not counters.

ab: plain, status and list decode of this tree's library and of --other (another build of the same ABI,
loaded through QPD_LIB), one fresh process per library and round, alternating; per call the rates of
both and the other build's own run-to-run spread.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, K, A, L, R = 1024, 512, 488, 8, 8
CHILD_LIMIT_S = 120


def setup(frames):
    import torch

    import bench

    w = bench.workload(N, K, L, "CA-SCL-LUT", frames, 2.0, luts="minsum")
    return w.dec, w.sym.to(torch.uint8).contiguous()


def timed(dec, fn):
    import torch

    dec.profile(True)
    dec.kernel_times()
    fn()
    torch.cuda.synchronize()
    kt = dec.kernel_times()
    dec.profile(False)
    return sum(ms for ms, _ in kt.values())


def calls(dec, x):
    import numpy as np

    masks = np.random.default_rng(7).integers(0, 2, size=(R, 16), dtype=np.uint8)
    out = {
        "plain": lambda: dec.decode_batch(x),
        "status": lambda: dec.decode_batch(x, return_status=True, crc_mask=masks[0]),
        "list": lambda: dec.decode_list_batch(x),
    }
    if hasattr(dec, "decode_search_batch"):
        out["search8"] = lambda: dec.decode_search_batch(x, masks)
        out["status_x8"] = lambda: [dec.decode_batch(x, return_status=True, crc_mask=m) for m in masks]
    return out


def summary(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run_search(args):
    dec, x = setup(args.frames)
    fns = calls(dec, x)
    for fn in fns.values():  # warm-up: allocations, first launches
        fn()
    ms = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            ms[k].append(timed(dec, fn))
    tail = {  # bytes written per frame besides the A output bytes (include/qpd.h)
        "search8": L * (4 + 8) + 4 + 4 + 8,
        "status_x8": R * (8 + 1) + (R - 1) * A,
        "list": L * (K + 9) + 4,
        "status": 8 + 1,
        "plain": 0,
    }
    for k in fns:
        s = summary(ms[k])
        print(json.dumps({"what": "mask_search", "call": k, "frames": args.frames, "rounds": args.rounds, "kernel_ms": s,
                          "frames_per_s": args.frames / s["median"] * 1e3, "tail_hbm_bytes_per_frame": tail[k] + A,
                          "code": f"CA-SCL-LUT N={N} A={A} K={K} L={L}", "masks": R if "8" in k else (1 if k == "status" else 0)}))


def run_child(args):
    dec, x = setup(args.frames)
    fns = {k: f for k, f in calls(dec, x).items() if k in ("plain", "status", "list")}
    for fn in fns.values():
        fn()
    print(json.dumps({k: timed(dec, fn) for k, fn in fns.items()}))


def run_ab(args):
    libs = {"this": None, "other": os.path.abspath(args.other)}
    ms = {name: {} for name in libs}
    for _ in range(args.rounds):
        for name, lib in libs.items():
            env = dict(os.environ)
            if lib:
                env["QPD_LIB"] = lib
            # one limit per child, sized to a 2^20-frame run (workload generation ~10 s, three calls < 1 s
            # each), enforced by timeout(1) with a kill behind it; after any child that faults, is killed
            # or times out nothing more is started on the device
            p = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "child",
                                "--frames", str(args.frames)], env=env, capture_output=True, text=True)
            if p.returncode:
                sys.stderr.write(p.stdout + p.stderr + f"\nchild ({name}) ended with status {p.returncode}: stopping\n")
                sys.exit(1)
            for k, v in json.loads(p.stdout.strip().splitlines()[-1]).items():
                ms[name].setdefault(k, []).append(v)
    for k in ms["this"]:
        t, o = summary(ms["this"][k]), summary(ms["other"][k])
        print(json.dumps({"what": "decode_ab", "call": k, "frames": args.frames, "rounds": args.rounds, "this_kernel_ms": t,
                          "other_kernel_ms": o, "this_over_other": t["median"] / o["median"],
                          "other_spread": (o["max"] - o["min"]) / o["median"],
                          "within_other_spread": o["min"] <= t["median"] <= o["max"]}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["search", "ab", "child"])
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--other")
    a = ap.parse_args()
    {"search": run_search, "ab": run_ab, "child": run_child}[a.mode](a)
