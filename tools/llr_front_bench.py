"""Measurements of the LLR front end of the LUT decoders (profiles/llr_front.jsonl), on the
bench workload's code (SCL-LUT, N = 1024, K = 512, L = 8, v = 16, MinDistortion tables and
channel quantizer) with 2^20 resident frames:

* front: kernel time of class 'pre' (qpd_profile / qpd_kernel_times) of
    - qpd_decode_u8          root_pre_kernel<uint8_t>, the yardstick (N bytes in, N out),
    - qpd_decode_llr f64/f32 llr_front_kernel in the pre-pass's place (8N / 4N bytes in, N out),
  for both read mappings of the front kernel (QPD_LLR_COOP = 1, the default, and 0), with the
  ratio to the yardstick, the ratio the bytes alone predict ((8N + N) / 2N = 4.5, (4N + N) / 2N
  = 2.5), the margin of 1.5x on top of it, and the achieved GB/s (bytes in + N bytes out);
* end_to_end: frames/s of whole calls (host clock around a call that ends in a device
  synchronise) of qpd_decode_u8, qpd_decode_llr f64 and f32 on the same frames -- reported,
  not gated.

One process, warm-up first, 7 alternating rounds, median [min, max].  Prints one JSON line per
measurement and appends them to --out.

    python tools/llr_front_bench.py --out profiles/llr_front.jsonl
"""
import argparse
import json
import os
import statistics
import sys
import time


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MARGIN = 1.5


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--K", type=int, default=512)
    ap.add_argument("--L", type=int, default=8)
    a = ap.parse_args()
    import torch

    assert torch.cuda.is_available(), "needs a HIP device"
    import quantized_decoder_polar_codes_amd as Q
    from quantized_decoder_polar_codes_amd import codes as C
    from quantized_decoder_polar_codes_amd import lutgen as LG
    from quantized_decoder_polar_codes_amd import montecarlo as MC

    N, K, L, B = a.N, a.K, a.L, a.frames
    _, mb, fm, _ = C.construct_pw(N, K)
    sigma = MC.sigma_for(2.0, K / N)
    packed = LG.design(N, 16, 3.0).packed()
    cq = Q.ChannelQuantizer.mindistortion(sigma, 128, 16)
    decs = {}
    for coop in (1, 0):  # read when the decoder is created
        os.environ["QPD_LLR_COOP"] = str(coop)
        decs[coop] = Q.from_packed("SCL-LUT", packed, K, fm, L=L)
    del os.environ["QPD_LLR_COOP"]
    info = decs[1].info()
    assert info["engine"] == 2, "the bench workload runs on the fast engine"
    _, llr64 = MC.GpuLlrFrames(decs[1], sigma, seed=1234)(0, B)
    llr32 = llr64.to(torch.float32)
    sym8 = decs[1].quantize_llr(llr64, cq)
    torch.cuda.synchronize()
    inputs = {"u8": sym8, "f64": llr64, "f32": llr32}
    in_bytes = {"u8": N, "f64": 8 * N, "f32": 4 * N}

    def call(dec, what):
        return dec.decode_batch(inputs[what]) if what == "u8" else dec.decode_llr_batch(inputs[what], cq)

    # the same bits from every way in, at the size that is timed
    ref = call(decs[1], "u8")
    for coop, dec in decs.items():
        for what in ("f64", "f32"):
            got = call(dec, what)
            same = torch.equal(got, ref) if what == "f64" else torch.equal(got, dec.decode_batch(dec.quantize_llr(llr32, cq)))
            assert same, (coop, what)
    cases = [("u8", 1), ("f64", 1), ("f32", 1), ("f64", 0), ("f32", 0)]

    def front_ms(what, coop):
        dec = decs[coop]
        dec.kernel_times()
        call(dec, what)
        torch.cuda.synchronize()
        ms, launches = dec.kernel_times()["pre"]
        assert launches == 1, launches
        return ms

    for dec in decs.values():
        dec.profile(True)
    for c in cases:  # warm-up: code objects, the allocator's blocks
        front_ms(*c)
    ms = {c: [] for c in cases}
    for _ in range(a.rounds):
        for c in cases:
            ms[c].append(front_ms(*c))
    for dec in decs.values():
        dec.profile(False)
    yard = statistics.median(ms[("u8", 1)])
    lines = []
    for what, coop in cases:
        med = statistics.median(ms[(what, coop)])
        byte_ratio = (in_bytes[what] + N) / (2 * N)
        ln = {"measurement": "front", "input": what, "N": N, "K": K, "L": L, "frames": B, "rounds": a.rounds,
              "kernel": "root_pre_kernel<uint8_t>" if what == "u8" else "llr_front_kernel",
              "pre_ms": summary(ms[(what, coop)]), "gb_per_s": B * (in_bytes[what] + N) / (med * 1e-3) / 1e9,
              "over_yardstick": med / yard, "byte_ratio": byte_ratio}
        if what != "u8":
            ln.update(mapping="cooperative" if coop else "per-owner", margin=MARGIN,
                      inside_margin=bool(med / yard <= MARGIN * byte_ratio))
        lines.append(ln)

    def timed(what):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call(decs[1], what)
        torch.cuda.synchronize()
        return B / (time.perf_counter() - t0)

    fps = {w: [] for w in inputs}
    for w in inputs:
        timed(w)
    for _ in range(a.rounds):
        for w in inputs:
            fps[w].append(timed(w))
    lines.append({"measurement": "end_to_end", "N": N, "K": K, "L": L, "frames": B, "rounds": a.rounds,
                  "frames_per_s": {w: summary(v) for w, v in fps.items()},
                  "llr_over_u8": {w: statistics.median(fps[w]) / statistics.median(fps["u8"]) for w in ("f64", "f32")}})
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
