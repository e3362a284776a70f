"""Measurements of the transmit side for caller-chosen messages (profiles/tx_frames.jsonl):

* tx_frames: tx_frames_kernel (qpd_tx_frames, int32 symbols and float64 LLRs, fed the
  generator's own messages) against mc_frames_kernel (qpd_mc_frames, qpd_mc_llr) on the same
  handle, kernel time by qpd_profile / qpd_kernel_times (class 'mc') -- C3's code
  (N = 1024, K = 512) at 2^20 frames and C2's (N = 128, K = 32) at 2^22;
* encode: tx_encode_kernel (qpd_encode, codeword only) on the same codes: kernel time,
  frames/s, and GB/s of A + N bytes per frame;
* encode_batch_host: decoder.encode_batch on 2^16 host frames (qpd_encode_host) against
  codes.polar_encode's host time.

One process, warm-up first, 7 alternating rounds, median [min, max].  Prints one JSON line
per measurement (and appends them to --out).

    python tools/tx_bench.py --out profiles/tx_frames.jsonl
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


def decoder(N, K):
    from quantized_decoder_polar_codes_amd import codes as C
    from quantized_decoder_polar_codes_amd.decoders import from_quant

    _, mb, fm, _ = C.construct_pw(N, K)
    return from_quant("SC", N, K, fm), mb


def tx_frames(N, K, frames, rounds):
    import torch

    from quantized_decoder_polar_codes_amd import montecarlo as MC
    from quantized_decoder_polar_codes_amd.decoders import ChannelQuantizer

    dec, _ = decoder(N, K)
    sigma = MC.sigma_for(2.0, K / N)
    qz = ChannelQuantizer.uniform(16, 0.5)
    sym_src = MC.GpuFrames(dec, qz.edges, qz.lut, 16, sigma, seed=1)
    llr_src = MC.GpuLlrFrames(dec, sigma, seed=1)
    llr_buf = torch.empty(frames * N, dtype=torch.float64, device=llr_src.device)
    msg, _ = sym_src(0, frames)  # the generator's messages of frames [0, frames): the same work per frame

    def run(mode):
        dec.kernel_times()
        if mode == "mc_frames":
            sym_src(0, frames)
        elif mode == "mc_llr":
            llr_src(0, frames, out=llr_buf)
        elif mode == "tx_symbols":
            dec.transmit_batch(msg, sigma, 1, quantizer=qz, out="symbols")
        else:
            dec.transmit_batch(msg, sigma, 1)
        torch.cuda.synchronize()
        ms, launches = dec.kernel_times()["mc"]
        assert launches == 1
        return ms

    modes = ("mc_frames", "tx_symbols", "mc_llr", "tx_llr")
    dec.profile(True)
    for mode in modes:  # warm-up: code objects, the allocator's blocks
        run(mode)
    ms = {m: [] for m in modes}
    for _ in range(rounds):
        for mode in modes:
            ms[mode].append(run(mode))
    dec.profile(False)
    med = {m: statistics.median(v) for m, v in ms.items()}
    return {"measurement": "tx_frames", "N": N, "K": K, "frames": frames, "rounds": rounds,
            "kernel_ms": {m: summary(v) for m, v in ms.items()},
            "tx_symbols_over_mc_frames": med["tx_symbols"] / med["mc_frames"], "tx_llr_over_mc_llr": med["tx_llr"] / med["mc_llr"]}


def encode(N, K, frames, rounds, hbm_tb_per_s):
    import torch

    dec, _ = decoder(N, K)
    msg = torch.randint(0, 2, (frames, K), dtype=torch.uint8, device="cuda")

    def run():
        dec.kernel_times()
        dec.encode_batch(msg)
        torch.cuda.synchronize()
        ms, launches = dec.kernel_times()["mc"]
        assert launches == 1
        return ms

    dec.profile(True)
    run()
    ms = [run() for _ in range(rounds)]
    dec.profile(False)
    med = statistics.median(ms) * 1e-3
    gbps = frames * (K + N) / med / 1e9
    return {"measurement": "encode", "N": N, "K": K, "frames": frames, "rounds": rounds, "kernel_ms": summary(ms),
            "frames_per_s": frames / med, "gb_per_s": gbps, "fraction_of_hbm": gbps / (hbm_tb_per_s * 1e3),
            "hbm_tb_per_s": hbm_tb_per_s}


def encode_batch_host(N, K, frames, rounds):
    from quantized_decoder_polar_codes_amd import codes as C

    dec, mb = decoder(N, K)
    msg = np.random.default_rng(1).integers(0, 2, size=(frames, K), dtype=np.uint8)

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return time.perf_counter() - t0, out

    lib_fn = lambda: dec.encode_batch(msg)  # noqa: E731
    np_fn = lambda: C.polar_encode(msg, mb, N)  # noqa: E731
    _, a = timed(lib_fn)
    _, b = timed(np_fn)
    assert (a == b).all()
    s = {"encode_batch": [], "polar_encode_numpy": []}
    for _ in range(rounds):
        s["encode_batch"].append(timed(lib_fn)[0])
        s["polar_encode_numpy"].append(timed(np_fn)[0])
    return {"measurement": "encode_batch_host", "N": N, "K": K, "frames": frames, "rounds": rounds,
            "seconds": {m: summary(v) for m, v in s.items()},
            "numpy_over_encode_batch": statistics.median(s["polar_encode_numpy"]) / statistics.median(s["encode_batch"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--scale", type=int, default=0, help="halve every frame count this many times (a quick look)")
    ap.add_argument("--hbm-tb-per-s", type=float, default=8.0, help="the device's peak HBM rate, for the encoder's fraction")
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "needs a HIP device"
    c3, c2, host = (1 << 20) >> a.scale, (1 << 22) >> a.scale, (1 << 16) >> a.scale
    lines = [tx_frames(1024, 512, c3, a.rounds), tx_frames(128, 32, c2, a.rounds),
             encode(1024, 512, c3, a.rounds, a.hbm_tb_per_s), encode(128, 32, c2, a.rounds, a.hbm_tb_per_s),
             encode_batch_host(1024, 512, host, a.rounds)]
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
