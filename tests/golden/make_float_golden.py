"""Generate the float-domain golden fixtures tests/golden/float_*.npz
(SCL, CA-SCL, FastSC, FastSCL, SC/SCL uniform-quantized,
SC/SCL Lloyd-quantized decoders).

Inputs are produced here (seeded numpy): either the reference driver's AWGN
channel (mainFPDecoder.py / mainQuantizedDecoder_ContinuousDomain.py: message,
polar encoding, BPSK, AWGN, LLR = 2y/sigma^2) or tie-heavy integer LLRs in
[-3, 3].  Expected outputs come from the REFERENCE decoders compiled from their
own sources under /root/reference (oracle/build_ref.sh -> oracle/_ref), one
``decode`` call per frame as the drivers do.  The re-quantizer parameters are
the simple Gaussian-approximation designs of quant.py (the reference's design
tools are offline scipy code, out of scope); decoder parity does not depend on
how they were designed.

GRID_CASES are cases in the style of tests/float_cases.py (non-nested frozen
masks, grid-aligned re-quantizers, frames on the grid) at N = 64, 32 frames each:
the first 31 frames of the case and its last one (the +-1e300 frame of the
re-quantized kinds).

Usage:  python tests/golden/make_float_golden.py      (needs oracle/_ref built)
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import oracle as O  # noqa: E402
from quantized_decoder_polar_codes_amd import codes as C  # noqa: E402
from test_float_oracle import CRC24, quant_for, ref_decoder  # noqa: E402

CASES = [
    # name, kind, N, K, L, style, B
    ("float_scl_n128_k64_l8_awgn", "SCL", 128, 64, 8, "awgn", 64),
    ("float_scl_n1024_k512_l8_awgn", "SCL", 1024, 512, 8, "awgn", 12),
    ("float_cascl_n128_a40_l8_awgn", "CA-SCL", 128, 64, 8, "awgn", 64),
    ("float_fastsc_n128_k64_ties", "FastSC", 128, 64, 1, "ties", 64),
    ("float_fastsc_n1024_k512_awgn", "FastSC", 1024, 512, 1, "awgn", 12),
    ("float_fastscl_n128_k64_l8_ties", "FastSCL", 128, 64, 8, "ties", 64),
    ("float_fastscl_n1024_k512_l8_awgn", "FastSCL", 1024, 512, 8, "awgn", 12),
    ("float_scuniform_n128_k64_awgn", "SC-Uniform", 128, 64, 1, "awgn", 64),
    ("float_scluniform_n128_k64_l4_awgn", "SCL-Uniform", 128, 64, 4, "awgn", 64),
    ("float_sclloyd_n128_k64_awgn", "SC-Lloyd", 128, 64, 1, "awgn", 64),
    ("float_scllloyd_n128_k64_l8_ties", "SCL-Lloyd", 128, 64, 8, "ties", 64),
]


GRID_CASES = [
    # name, kind, mask, L, quantizer (float_cases.Case.quant), seed of the frames
    ("float_scuniform_n64_info0_r49_64_v15", "SC-Uniform", "info0", 1, ("grid", 49.0 / 64.0, 15), 301),
    ("float_scluniform_n64_block2_l8_r025_v2", "SCL-Uniform", "block2", 8, ("grid", 0.25, 2), 302),
    ("float_sclloyd_n64_random_ragged", "SC-Lloyd", "random", 1, ("lloyd", 303, True), 303),
    ("float_scllloyd_n64_random_l4_unsorted", "SCL-Lloyd", "random", 4, ("unsorted", 304), 304),
    ("float_fastscl_n64_block2_l8_grid", "FastSCL", "block2", 8, (), 305),
    ("float_cascl_n64_frozen_last_l8_grid", "CA-SCL", "frozen_last", 8, (), 306),
]


def save(name, kind, N, K, L, fm, nt, llr, expected, q, A=None, crc=None):
    rec = dict(kind=np.array(kind), N=N, K=K, L=L, frozen=np.asarray(fm).astype(np.int32), node_type=nt, llr=llr,
               expected=expected)
    if q is not None:
        rec["v"] = q.v
        if hasattr(q, "r_f"):
            rec.update(r_f=q.r_f, r_g=q.r_g)
        else:
            rec.update(bnd=q.bnd, bnd_off=q.bnd_off, bnd_len=q.bnd_len, rec=q.rec, rec_off=q.rec_off,
                       rec_len=q.rec_len)
    if crc is not None:
        rec.update(A=A, crc_n=crc[0], crc_loc=np.array(crc[1], dtype=np.int32))
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **rec)
    print(f"{name}: {len(llr)} frames, {int(expected.size)} bits")


def grid_main(R):
    import float_cases as F

    for name, kind, mask, L, quant, seed in GRID_CASES:
        c = F.Case(kind, 64, mask, L, quant, seed)
        fm, nt, K = F.code_of(c.N, c.mask)
        assert not F._root_refused(kind, nt), name
        q = F.quant_of(c)
        llr = np.ascontiguousarray(F.frames_of(c)[np.r_[0:31, F.B - 1]])
        kw = F.decoder_kw(c)
        A, crc = (kw["A"], (kw["crc_n"], kw["crc_loc"])) if kw else (None, None)
        d = ref_decoder(R, kind, c.N, K, L, fm.tolist(), (1 - fm).tolist(), nt.tolist(), q, A, crc)
        expected = np.stack([d.decode(x[None]) for x in llr]).astype(np.uint8)
        save(name, kind, c.N, K, L, fm, nt, llr, expected, q, A, crc)


def inputs(N, K, msgbits, B, style, seed, ebn0_db=1.5):
    rng = np.random.default_rng(seed)
    if style == "ties":
        return rng.integers(-3, 4, size=(B, N)).astype(np.float64)
    rate = K / N
    sigma = np.sqrt(1 / (2 * rate * 10 ** (ebn0_db / 10)))
    msg = rng.integers(0, 2, size=(B, K), dtype=np.uint8)
    x = C.polar_encode(msg, msgbits, N)
    y = (1.0 - 2.0 * x) + rng.normal(0, sigma, size=(B, N))
    return y * 2 / sigma ** 2


def main():
    R = O.reference_module()
    if R is None or not hasattr(R, "SCLDecoder"):
        raise SystemExit("oracle/_ref not built (run oracle/build_ref.sh)")
    for i, (name, kind, N, K, L, style, B) in enumerate(CASES):
        _, mb, fm, mm = C.construct_pw(N, K)
        nt = C.identify_nodes(N, mb).astype(np.int32)
        q = quant_for(kind, N)
        llr = inputs(N, K, mb, B, style, seed=9000 + i)
        A, crc = None, None
        if kind == "CA-SCL":
            A, crc = 40, (24, CRC24)
        d = ref_decoder(R, kind, N, K, L, fm.tolist(), mm.tolist(), nt.tolist(), q, A, crc)
        expected = np.stack([d.decode(x[None]) for x in llr]).astype(np.uint8)
        save(name, kind, N, K, L, fm, nt, llr, expected, q, A, crc)
    grid_main(R)


if __name__ == "__main__":
    main()
