"""Shared by the transmit side's tests (tests/test_encode_host.py, test_polarbdenc.py,
test_gpu_encode.py, test_gpu_tx_frames.py): the CPU harness's runner
(tests/native/tx_harness.cpp), the numpy reference of the encoder -- codes.polar_encode
of the message and the first K - A bits of (oracle.crc_encode ^ the placed mask) -- the
restatement of the channel for a given codeword, and the committed RNTI round-trip case."""
import os
import subprocess

import numpy as np

import code_masks as M
import mc_ref
from conftest import ROOT

CSRC = os.path.join(ROOT, "quantized_decoder_polar_codes_amd", "csrc")
BUILD = os.path.join(ROOT, "tests", "_build")
CRC24_LOC = (24, 23, 21, 20, 17, 15, 13, 12, 8, 4, 2, 1, 0)
QPD_E_INVALID, QPD_E_UNSUPPORTED = -1, -2
ERR_MSG_BIT = 16
KIND = {"SC": 0, "SC-LUT": 1, "SCL-LUT": 2, "CA-SCL-LUT": 5, "CA-FastSCL-LUT": 6, "SCL": 7, "CA-SCL": 8, "FastSC": 9}

# The RNTI round trip (CA-SCL float, K - A = 24, L = 8, 256 frames): messages of seed RNTI_SEED encoded
# under RNTI_MASK.  Decoded noiselessly under RNTI_MASK every frame passes; under RNTI_OTHER none does --
# a property of these inputs (no other list candidate of any of the 256 frames carries a CRC that fits
# the other mask), confirmed with the host engine and the oracle's CRC for this seed.
RNTI_N, RNTI_A, RNTI_L, RNTI_SEED, RNTI_FRAMES = 128, 40, 8, 20261021, 256
RNTI_MASK = np.array([1, 0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0, 1, 0, 1], dtype=np.uint8)
RNTI_OTHER = np.array([0, 1, 1, 0, 1, 0, 0, 1, 0, 0, 1, 1, 1, 0, 1, 0], dtype=np.uint8)


def rnti_case():
    """(frozen mask, messages [256, A]) of the committed round trip."""
    from quantized_decoder_polar_codes_amd import codes as C

    _, _, fm, _ = C.construct_pw(RNTI_N, RNTI_A + 24)
    msg = np.random.default_rng(RNTI_SEED).integers(0, 2, size=(RNTI_FRAMES, RNTI_A), dtype=np.uint8)
    return np.asarray(fm, dtype=np.int32), msg


def build_harness(sanitize=False):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "tx_harness")
    src = os.path.join(ROOT, "tests", "native", "tx_harness.cpp")
    deps = [src, os.path.join(ROOT, "include", "qpd.h")] + [
        os.path.join(CSRC, f) for f in ("qpd_tx.hpp", "qpd_status.hpp", "qpd_config.hpp", "qpd_host.hpp", "qpd_schedule.hpp",
                                        "qpd_types.hpp", "stl_sort.hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", CSRC, src, "-o", exe + ".tmp"],
                       check=True)
        os.replace(exe + ".tmp", exe)
    return exe


def run_harness(exe, tmp_path, mode, kind, fm, msg=None, A=None, crc_n=24, crc_loc=CRC24_LOC, B=None, mask=None,
                null_mask=False, mask_bits=None, want_info=True, want_cw=True, no_signal=0, null_msg=False, out_type=2,
                has_ch=True, q=16, has_rec=False, null_frames=False, frames_offset=0, frame0=0, L=1, dec_mask=None,
                node_type=None):
    """One harness run -> dict(rc, flag, msg (the refusal's text), info, cw, bits, passed)."""
    fm = np.asarray(fm)
    N, K = fm.size, int((fm == 0).sum())
    ca = kind in (5, 6, 8)
    Am = A if ca else K
    msg = np.zeros((0, Am), np.uint8) if msg is None else np.ascontiguousarray(np.asarray(msg, dtype=np.uint8).reshape(-1, Am))
    B = len(msg) if B is None else B
    mb = -1 if mask is None and mask_bits is None else (len(mask) if mask_bits is None else mask_bits)
    mask = np.zeros(0, np.uint8) if mask is None else np.asarray(mask, dtype=np.uint8)
    dec_mask = np.zeros(0, np.uint8) if dec_mask is None else np.asarray(dec_mask, dtype=np.uint8)
    h = [mode, kind, N, K, A or 0, crc_n, len(crc_loc), B, mb, int(null_mask), int(want_info), int(want_cw), no_signal,
         int(null_msg), out_type, int(has_ch), q, int(has_rec), int(null_frames), frames_offset, frame0, L, len(dec_mask),
         int(node_type is not None)]
    case, res = str(tmp_path / "tx_case.bin"), str(tmp_path / "tx_result.bin")
    with open(case, "wb") as f:
        f.write(np.array(h, dtype="<i4").tobytes())
        f.write(fm.astype("<i4").tobytes())
        f.write(np.asarray(crc_loc, dtype="<i4").tobytes())
        f.write(np.resize(mask, max(mb, 0)).astype(np.uint8).tobytes() if mb > 0 and len(mask) else b"\0" * max(mb, 0))
        f.write(dec_mask.tobytes())
        f.write(np.resize(msg, (max(B, 0), Am)).tobytes() if len(msg) else b"\0" * (max(B, 0) * Am))
        if node_type is not None:
            f.write(np.asarray(node_type, dtype="<i4").tobytes())
    p = subprocess.run([exe, case, res], check=True, capture_output=True, text=True)
    raw = open(res, "rb").read()
    rc, flag = (int(x) for x in np.frombuffer(raw[:8], dtype="<i4"))
    out = dict(rc=rc, flag=flag, msg=p.stdout.strip(), info=None, cw=None, bits=None, passed=None)
    body = np.frombuffer(raw[8:], dtype=np.uint8)
    if rc == 0 and mode == 0 and B > 0:
        at = 0
        if want_info:
            out["info"], at = body[: B * K].reshape(B, K), B * K
        if want_cw:
            out["cw"] = body[at: at + B * N].reshape(B, N)
    if rc == 0 and mode == 2:
        out["bits"], out["passed"] = body[: B * Am].reshape(B, Am), body[B * Am:]
    return out


def placed_mask(mask, crc_n):
    """The mask as a [crc_n] row: mask bit l on check-code bit crc_n - len(mask) + l."""
    row = np.zeros(crc_n, dtype=np.uint8)
    if mask is not None and len(mask):
        row[crc_n - len(mask):] = mask
    return row


def encode_ref(fm, msg, A=None, crc_n=24, crc_loc=CRC24_LOC, mask=None):
    """(info, codeword) by codes.polar_encode and, with A, oracle.crc_encode."""
    import oracle
    from quantized_decoder_polar_codes_amd import codes as C

    fm = np.asarray(fm)
    N, mb = fm.size, np.flatnonzero(fm == 0)
    msg = np.asarray(msg, dtype=np.uint8) & 1
    info = msg
    if A is not None:
        info = np.concatenate([msg, (oracle.crc_encode(msg, crc_n, crc_loc) ^ placed_mask(mask, crc_n))[:, : mb.size - A]], axis=1)
    return info, C.polar_encode(info, mb, N)


def mask_for(N, name, K=None):
    """A frozen mask by name: "random" with K information positions, else code_masks.named_mask."""
    if name == "random":
        return M.random_mask(N, K if K is not None else N // 2, N + 7)
    return M.named_mask(N, name)


def llr_ref(x, seed, frame0, sigma, signal=True):
    """tests/mc_ref.py's channel for the codewords x [B, N]: the LLRs of frames frame0 .. frame0 + B."""
    x = np.asarray(x)
    B, N = x.shape
    gid = np.arange(B, dtype=np.uint64) + np.uint64(frame0)
    glo, ghi = gid & np.uint64(mc_ref.MASK), gid >> np.uint64(32)
    slo, shi = seed & mc_ref.MASK, (seed >> 32) & mc_ref.MASK
    llr = np.zeros((B, N), dtype=np.float64)
    inv_s2 = 1.0 / (np.float64(sigma) * np.float64(sigma))
    for p in range(N // 2):
        r = mc_ref.philox(glo, ghi, np.full(B, p, np.uint64), np.full(B, mc_ref.TAG_NOISE, np.uint64), slo, shi)
        u1 = 2.0 - mc_ref.one_m(r[0], r[1])
        u2 = mc_ref.one_m(r[2], r[3]) - 1.0
        rad = np.sqrt(-2.0 * np.log(u1))
        ang = 6.283185307179586 * u2
        nz = (rad * np.cos(ang), rad * np.sin(ang))
        for h in range(2):
            e = 2 * p + h
            y = np.float64(sigma) * nz[h]
            if signal:
                y = (1.0 - 2.0 * x[:, e].astype(np.float64)) + y
            llr[:, e] = y * 2.0 * inv_s2
    return llr
