"""Measurements of the float64-LLR Monte-Carlo front end (profiles/mc_llr.jsonl):

* generator: mc_frames_kernel in LLR mode (qpd_mc_llr, no rec) against the int32
  symbol mode (qpd_mc_frames), kernel time by qpd_profile / qpd_kernel_times
  (class 'mc') for 2^20 frames at N = 1024;
* end_to_end: GpuLlrFrames.decode_frames (generate + decode + count) against
  decode_batch on resident LLRs, frames/s at 2^15 frames, float SCL (L = 8) and
  float FastSC at N = 1024, K = 512.

One process, warm-up first, 7 alternating rounds, median [min, max].  Prints one
JSON line per measurement (and appends them to --out).

    python tools/mc_llr_bench.py --out profiles/mc_llr.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def code(N, K):
    from quantized_decoder_polar_codes_amd import codes as C

    _, mb, fm, _ = C.construct_pw(N, K)
    return fm, C.identify_nodes(N, mb).astype(np.int32)


def generator(frames, rounds, N=1024, K=512):
    import torch

    from quantized_decoder_polar_codes_amd import montecarlo as MC
    from quantized_decoder_polar_codes_amd.decoders import from_quant

    fm, nt = code(N, K)
    dec = from_quant("SC", N, K, fm)
    sigma = MC.sigma_for(2.0, K / N)
    edges, lut = MC.uniform_channel_quantizer(16, 0.5)
    sym_src = MC.GpuFrames(dec, edges, lut, 16, sigma, seed=1)
    llr_src = MC.GpuLlrFrames(dec, sigma, seed=1)
    llr_buf = torch.empty(frames * N, dtype=torch.float64, device=llr_src.device)

    def run(mode, f0):
        dec.kernel_times()
        if mode == "llr":
            llr_src(f0, frames, out=llr_buf)
        else:
            sym_src(f0, frames)
        torch.cuda.synchronize()
        ms, launches = dec.kernel_times()["mc"]
        assert launches == 1
        return ms

    dec.profile(True)
    for mode in ("int32", "llr"):  # warm-up: code objects, the allocator's blocks
        run(mode, 0)
    ms = {"int32": [], "llr": []}
    for r in range(rounds):
        for mode in ("int32", "llr"):
            ms[mode].append(run(mode, (r + 1) * frames))
    dec.profile(False)
    return {"measurement": "generator", "N": N, "K": K, "frames": frames, "rounds": rounds,
            "kernel_ms": {m: summary(v) for m, v in ms.items()},
            "store_tb_per_s_llr": frames * N * 8 / (statistics.median(ms["llr"]) * 1e-3) / 1e12,
            "llr_over_int32": statistics.median(ms["llr"]) / statistics.median(ms["int32"])}


def end_to_end(kind, L, frames, rounds, N=1024, K=512):
    import torch

    from quantized_decoder_polar_codes_amd import montecarlo as MC
    from quantized_decoder_polar_codes_amd.decoders import from_quant

    fm, nt = code(N, K)
    dec = from_quant(kind, N, K, fm, L=L, node_type=nt)
    src = MC.GpuLlrFrames(dec, MC.sigma_for(2.0, K / N), seed=1)
    counts = torch.zeros(2, dtype=torch.int64, device=src.device)
    _, llr = src(0, frames)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return frames / (time.perf_counter() - t0)

    fused = lambda: src.decode_frames(0, frames, counts=counts)  # noqa: E731
    resident = lambda: dec.decode_batch(llr)  # noqa: E731
    for fn in (fused, resident):
        timed(fn)
    fps = {"decode_frames": [], "decode_batch_resident": []}
    for _ in range(rounds):
        fps["decode_frames"].append(timed(fused))
        fps["decode_batch_resident"].append(timed(resident))
    return {"measurement": "end_to_end", "kind": kind, "N": N, "K": K, "L": L, "frames": frames, "rounds": rounds,
            "frames_per_s": {m: summary(v) for m, v in fps.items()},
            "fused_over_resident": statistics.median(fps["decode_frames"]) /
            statistics.median(fps["decode_batch_resident"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--gen-frames", type=int, default=1 << 20)
    ap.add_argument("--e2e-frames", type=int, default=1 << 15)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "needs a HIP device"
    lines = [generator(a.gen_frames, a.rounds), end_to_end("SCL", 8, a.e2e_frames, a.rounds),
             end_to_end("FastSC", 1, a.e2e_frames, a.rounds)]
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
