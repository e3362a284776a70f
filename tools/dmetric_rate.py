"""Rates of the blind-detection metric (qpd_dmetric, profiles/dmetric.jsonl) on one float FastSC decoder in
one process per workload, on resident float64 LLRs (2^20 frames, AWGN at 2 dB from the library's generator):

    dmetric        FastSCDecoder.dmetric_batch(llr)                    the metric alone
    dmetric_bits   FastSCDecoder.dmetric_batch(llr, return_bits=True)  metric and bits
    decode         FastSCDecoder.decode_batch(llr)                     the plain float FastSC kernel

A warm-up of each, then --repeats rounds that alternate the three calls (so drift hits all alike); HIP events
around each call; median [min, max] of the frames/s.  Also the host engine's time per frame (qpd_dmetric_host,
one frame per call, host engine forced).  One JSON line per workload and call.

    python tools/dmetric_rate.py --workload 0 --out profiles/dmetric.jsonl        N = 512, K = 100
    python tools/dmetric_rate.py --workload 1 --out profiles/dmetric.jsonl        N = 128, K = 64
    python tools/dmetric_rate.py --workload 0 --only decode --label parent        the plain path alone (A/B of
                                                                                  two builds, QPD_LIB)
    python tools/dmetric_rate.py --reference --out profiles/dmetric.jsonl         no GPU: the reference's
        DMetricCalculator.calculate per frame, built as tests/golden/make_dmetric_golden.py builds it
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = [(512, 100), (128, 64)]


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def code(N, K):
    from quantized_decoder_polar_codes_amd import codes as C

    _, mb, fm, mm = C.construct_pw(N, K)
    return fm, mm, C.identify_nodes(N, mb).astype(np.int32)


def reference(out):
    """The reference's calculate() per frame on this machine's CPU (no GPU involved)."""
    import tempfile

    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_dmetric_golden as G

    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        R = G.reference_dmetric(tmp)
        for N, K in WORKLOADS:
            fm, mm, nt = code(N, K)
            d = R.DMetricCalculator(N, K, fm.astype(int).tolist(), mm.astype(int).tolist(), nt.astype(int).tolist())
            llr = np.random.default_rng(1).normal(1.0, 1.2, size=(2000, 1, N))
            for x in llr[:200]:
                d.calculate(x)
            us = []
            for _ in range(7):
                t0 = time.perf_counter()
                for x in llr:
                    d.calculate(x)
                us.append((time.perf_counter() - t0) / len(llr) * 1e6)
            lines.append({"what": "reference_calculate", "N": N, "K": K, "us_per_frame": spread(us),
                          "where": "the CPU of the machine the reference was built on, one core; not the GPU host"})
    emit(lines, out)


def emit(lines, out):
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--only", default=None, help="measure this call alone (decode: the plain path, any build)")
    ap.add_argument("--label", default="this", help="the build's name in the record (with QPD_LIB: parent)")
    ap.add_argument("--reference", action="store_true")
    a = ap.parse_args()
    if a.reference:
        return reference(a.out)
    import torch

    from quantized_decoder_polar_codes_amd import montecarlo as MC
    from quantized_decoder_polar_codes_amd.decoders import FastSCDecoder

    assert torch.cuda.is_available(), "needs a HIP device"
    N, K = WORKLOADS[a.workload]
    fm, mm, nt = code(N, K)
    dec = FastSCDecoder(N, K, fm, mm, nt)
    _, llr = MC.GpuLlrFrames(dec, MC.sigma_for(2.0, K / N), seed=1)(0, a.frames)
    llr = llr.reshape(a.frames, N)
    calls = {"dmetric": lambda: dec.dmetric_batch(llr), "dmetric_bits": lambda: dec.dmetric_batch(llr, return_bits=True),
             "decode": lambda: dec.decode_batch(llr)}
    if a.only:
        calls = {a.only: calls[a.only]}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), r

    digest = {}
    for tag, fn in calls.items():  # warm-up: code objects resident, the allocator's blocks; and the results
        for _ in range(2):
            _, r = timed(fn)
        digest[tag] = [hashlib.sha1(t.cpu().numpy().tobytes()).hexdigest()[:12] for t in (r if isinstance(r, tuple) else (r,))]
    if not a.only:
        assert digest["dmetric"][0] == digest["dmetric_bits"][0] and digest["dmetric_bits"][1] == digest["decode"][0], digest
    ms = {t: [] for t in calls}
    for _ in range(a.repeats):
        for tag, fn in calls.items():
            ms[tag].append(timed(fn)[0])
    base = {"N": N, "K": K, "frames": a.frames, "build": a.label, "device": torch.cuda.get_device_name(0)}
    lines = [dict(base, what=tag, ms=spread(ms[tag]), mframes_per_s=spread([a.frames / x / 1e3 for x in ms[tag]]),
                  digest=digest[tag]) for tag in calls]
    if not a.only:  # the per-frame call on the host engine
        dec.set_host_engine("cpu")
        x = llr[:2000].cpu().numpy()
        us = []
        for r in range(a.repeats + 1):
            t0 = time.perf_counter()
            for row in x:
                dec.dmetric_batch(row)
            if r:
                us.append((time.perf_counter() - t0) / len(x) * 1e6)
        lines.append(dict(base, what="host_engine_per_frame", frames=len(x), us_per_frame=spread(us),
                          where="the GPU machine's host CPU, one core, through FastSCDecoder.dmetric_batch"))
    emit(lines, a.out)


if __name__ == "__main__":
    main()
