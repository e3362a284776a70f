"""Build and load helper of the Monte-Carlo arithmetic harness (tests/native/mc_math_harness.hip):
libmc_math_harness.so under tests/_build/, compiled with build.py's compiler, target, flags and
include paths and stamped with a hash of the harness and of every file under csrc/ (as
tests/sel_harness.py does), so that it is rebuilt only when one of them changed.
__graft_entry__.build() builds it with the rest; tests/test_gpu_mc_math.py loads it."""
from __future__ import annotations

import ctypes
import hashlib
import os
import subprocess

import numpy as np

from quantized_decoder_polar_codes_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "mc_math_harness.hip")
OUT_DIR = os.path.join(HERE, "_build")
LIB = os.path.join(OUT_DIR, "libmc_math_harness.so")
TAG = b"qpd-mcm-build-id:"

FIELDS = ("u1", "u2", "log", "sin", "cos", "nz0", "nz1")


def source_hash() -> str:
    h = hashlib.sha256()
    h.update(repr((B.ARCH, B.COMMON_FLAGS)).encode())
    for path in [SRC] + B._sources():
        h.update(os.path.relpath(path, B.ROOT).encode() + b"\0")
        with open(path, "rb") as f:
            h.update(f.read())
        h.update(b"\0")
    return h.hexdigest()[:32]


def library_build_id(path: str = LIB) -> str | None:
    try:
        with open(path, "rb") as f:
            data = f.read()
    except OSError:
        return None
    i = data.find(TAG)
    return None if i < 0 else data[i + len(TAG): i + len(TAG) + 32].decode("ascii", "replace")


def needs_build() -> bool:
    return library_build_id() != source_hash()


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not needs_build():
        return LIB
    os.makedirs(OUT_DIR, exist_ok=True)
    cmd = [B.HIPCC, f"--offload-arch={B.ARCH}"] + B.COMMON_FLAGS + [
        "-I", os.path.join(B.ROOT, "include"), "-I", B.SRC, f'-DQPD_MCM_BUILD_ID="{source_hash()}"',
        "-shared", SRC, "-o", LIB + ".tmp"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    os.replace(LIB + ".tmp", LIB)
    return LIB


_U32 = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
_F64 = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")


class Harness:
    def __init__(self, path: str):
        lib = ctypes.CDLL(path)
        lib.qpd_mcm_build_id.restype = ctypes.c_char_p
        lib.qpd_mcm_noise.argtypes = [ctypes.c_int64, _U32, _U32, _U32, _U32, _F64]
        lib.qpd_mcm_philox.argtypes = [ctypes.c_int, ctypes.c_int, _U32, _U32, _U32]
        self.lib = lib
        self.build_id = lib.qpd_mcm_build_id().decode()

    def noise(self, a, b, c, d) -> dict:
        """The generator's noise step on the Philox words (a, b, c, d), uint32 [n]: {field: float64 [n]}
        for FIELDS -- u1 = 2 - 1.(a >> 12 : b), u2 = 1.(c >> 12 : d) - 1, mc_log(u1), sin and cos of
        6.283185307179586 * u2, and the two Gaussians."""
        a, b, c, d = (np.ascontiguousarray(x, np.uint32) for x in (a, b, c, d))
        n = a.size
        assert b.size == n and c.size == n and d.size == n
        out = np.empty((7, n), np.float64)
        rc = self.lib.qpd_mcm_noise(n, a, b, c, d, out)
        assert rc == 0, f"qpd_mcm_noise: error {rc}"
        return dict(zip(FIELDS, out))

    def philox(self, keys, ctr):
        """philox4x32_10 of ctr (uint32 [nk, nc, 4]) under keys (uint32 [nk, 2]): uint32 [nk, nc, 4]."""
        keys = np.ascontiguousarray(keys, np.uint32)
        ctr = np.ascontiguousarray(ctr, np.uint32)
        nk, nc = ctr.shape[:2]
        assert keys.shape == (nk, 2) and ctr.shape == (nk, nc, 4)
        out = np.empty(ctr.shape, np.uint32)
        rc = self.lib.qpd_mcm_philox(nk, nc, keys, ctr, out)
        assert rc == 0, f"qpd_mcm_philox: error {rc}"
        return out


def load() -> Harness:
    h = Harness(build())
    if h.build_id != source_hash():
        raise RuntimeError(f"{LIB} carries build id {h.build_id}, the tree hashes to {source_hash()}")
    return h
