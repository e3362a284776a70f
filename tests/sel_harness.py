"""Build and load helper of the survivor-selection harness (tests/native/sel_harness.hip):
libsel_harness.so under tests/_build/, compiled with build.py's compiler, target, flags
and include paths and stamped with a hash of the harness and of every file under csrc/
(as build.py stamps libqpd.so), so that it is rebuilt only when one of them changed.
__graft_entry__.build() builds it with the rest; tests/test_gpu_selection.py loads it."""
from __future__ import annotations

import ctypes
import hashlib
import os
import subprocess

import numpy as np

from quantized_decoder_polar_codes_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "sel_harness.hip")
OUT_DIR = os.path.join(HERE, "_build")
LIB = os.path.join(OUT_DIR, "libsel_harness.so")
TAG = b"qpd-sel-build-id:"

# the primitives (enum Prim of the harness)
GENERIC, SEL8, SEL16, SEL16_SERIAL, KEEP8, KEEP16 = range(6)


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
        "-I", os.path.join(B.ROOT, "include"), "-I", B.SRC, f'-DQPD_SEL_BUILD_ID="{source_hash()}"',
        "-shared", SRC, "-o", LIB + ".tmp"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    os.replace(LIB + ".tmp", LIB)
    return LIB


_F64 = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_I32 = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_U8 = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")


class Harness:
    def __init__(self, path: str):
        lib = ctypes.CDLL(path)
        lib.qpd_sel_build_id.restype = ctypes.c_char_p
        lib.qpd_sel_group_size.argtypes = [ctypes.c_int, ctypes.c_int]
        lib.qpd_sel_run.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _F64, _F64, ctypes.c_void_p,
                                    _I32, _I32, _I32, _I32]
        lib.qpd_sel_reference.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64, _F64, _F64, _I32, _I32]
        lib.qpd_sel_fallback.argtypes = [ctypes.c_int, ctypes.c_int64, _F64, _F64, _U8, _I32]
        lib.qpd_sel_adversary.argtypes = [ctypes.c_int, _F64]
        self.lib = lib
        self.build_id = lib.qpd_sel_build_id().decode()

    def group_size(self, prim: int, L: int) -> int:
        return int(self.lib.qpd_sel_group_size(prim, L))

    def run_raw(self, prim, L, nsets, nblocks, keep, flip, force=None):
        """The entry point's return code alone (argument validation)."""
        n = max(1, nblocks) * max(1, nsets) * 64
        out = [np.zeros(n, np.int32) for _ in range(3)] + [np.zeros(max(1, nblocks), np.int32)]
        fp = None if force is None else force.ctypes.data_as(ctypes.c_void_p)
        return int(self.lib.qpd_sel_run(prim, L, nsets, nblocks, keep, flip, fp, *out))

    def run(self, prim, L, keep, flip, force=None):
        """keep, flip: float64 [blocks, sets, 64]; force: uint8 [blocks, sets] group masks
        (SEL16_SERIAL).  Returns parent, upper, ident ([blocks, sets, 64]) and the blocks'
        canary flags."""
        keep = np.ascontiguousarray(keep, np.float64)
        flip = np.ascontiguousarray(flip, np.float64)
        assert keep.shape == flip.shape and keep.ndim == 3 and keep.shape[2] == 64, keep.shape
        nb, ns = keep.shape[:2]
        parent, upper, ident = (np.empty(keep.shape, np.int32) for _ in range(3))
        canary = np.empty(nb, np.int32)
        fp = None
        if force is not None:
            force = np.ascontiguousarray(force, np.uint8)
            assert force.shape == (nb, ns)
            fp = force.ctypes.data_as(ctypes.c_void_p)
        rc = self.lib.qpd_sel_run(prim, L, ns, nb, keep, flip, fp, parent, upper, ident, canary)
        assert rc == 0, f"qpd_sel_run: error {rc}"
        return parent, upper, ident, canary

    def reference(self, L, gs, keep, flip):
        """mink (std::sort on the 2L candidate indices, first L) per lane group: parent,
        upper in the shape of keep; -1 on the padding lanes gl >= L."""
        keep = np.ascontiguousarray(keep, np.float64)
        flip = np.ascontiguousarray(flip, np.float64)
        parent, upper = np.empty(keep.shape, np.int32), np.empty(keep.shape, np.int32)
        rc = self.lib.qpd_sel_reference(L, gs, keep.size // 64, keep, flip, parent, upper)
        assert rc == 0
        return parent, upper

    def fallback(self, L, keep, flip):
        """Per group of 16 ([..., 4]): does the replay reach the introsort's depth limit,
        and the partitions it ran."""
        keep = np.ascontiguousarray(keep, np.float64)
        flip = np.ascontiguousarray(flip, np.float64)
        shape = keep.shape[:-1] + (4,)
        fell, parts = np.empty(shape, np.uint8), np.empty(shape, np.int32)
        rc = self.lib.qpd_sel_fallback(L, keep.size // 64, keep, flip, fell, parts)
        assert rc == 0
        return fell.astype(bool), parts

    def adversary(self, n):
        """The keys McIlroy's adversary settles on against std::sort of n elements."""
        out = np.empty(n, np.float64)
        assert self.lib.qpd_sel_adversary(n, out) == 0
        return out


def load() -> Harness:
    h = Harness(build())
    if h.build_id != source_hash():
        raise RuntimeError(f"{LIB} carries build id {h.build_id}, the tree hashes to {source_hash()}")
    return h
