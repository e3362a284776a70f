"""int32 against uint8 channel symbols on one decoder in one process (qpd_decode / qpd_decode_u8 through
decode_batch on device tensors), for the bench workloads C3 (SCL-LUT N=1024 K=512 L=8) and C2 (SC-LUT N=128
K=32): the root pre-pass kernel time (profile() / kernel_times()['pre']) and the end-to-end frames/s.

Per workload: the same frames as int32 and as uint8, a warm-up of each, then REPEATS rounds that alternate
the two inputs (so drift hits both alike); the kernel-time rounds run with profiling on, the throughput
rounds with it off (the events of profile() would sit inside the timed span).  One JSON line per workload and
input with median, min and max over the rounds, and the decoded bits' digest (equal for both inputs).
usage: python tools/u8_input_ab.py [--out profiles/u8_input_ab.jsonl] [--repeats 7]"""
import argparse
import hashlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

WORKLOADS = [("C3", "SCL-LUT", 1024, 512, 8, 1 << 20), ("C2", "SC-LUT", 128, 32, 1, 1 << 22)]


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def timed(dec, x):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    dec.decode_batch(x)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "u8_input_ab.jsonl"))
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--scale", type=float, default=1.0, help="frames per workload, as a fraction of the default")
    args = ap.parse_args()
    lines = []
    for name, kind, N, K, L, frames in WORKLOADS:
        frames = max(1024, int(frames * args.scale))
        wl = bench.workload(N, K, L, kind, frames, 2.0)
        dec = wl.dec
        inputs = {"int32": wl.sym, "uint8": wl.sym.to(torch.uint8)}
        digest = {}
        for tag, x in inputs.items():  # warm-up: buffers grown, code resident; and the bits
            for _ in range(2):
                out = dec.decode_batch(x)
            torch.cuda.synchronize()
            digest[tag] = hashlib.sha1(out.cpu().numpy().tobytes()).hexdigest()[:12]
            staged = dec.info()["u8_staged"]
            assert staged == 0, "the A/B is about the direct path"
        assert digest["int32"] == digest["uint8"], digest
        pre = {t: [] for t in inputs}
        wall = {t: [] for t in inputs}
        dec.profile(True)
        dec.kernel_times()
        for _ in range(args.repeats):
            for tag, x in inputs.items():
                dec.decode_batch(x)
                pre[tag].append(dec.kernel_times()["pre"][0])
        dec.profile(False)
        for _ in range(args.repeats):
            for tag, x in inputs.items():
                wall[tag].append(timed(dec, x))
        for tag in inputs:
            lines.append({"workload": name, "kind": kind, "N": N, "K": K, "L": L, "frames": frames, "input": tag,
                          "input_bytes": int(inputs[tag].numel() * inputs[tag].element_size()),
                          "pre_ms": spread(pre[tag]), "decode_batch_ms": spread(wall[tag]),
                          "mframes_per_s": spread([frames / ms / 1e3 for ms in wall[tag]]),
                          "digest": digest[tag], "device": torch.cuda.get_device_name(0)})
            print(json.dumps(lines[-1]), flush=True)
        del wl, dec, inputs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
