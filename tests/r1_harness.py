"""Build and load helper of the R1-node harness (tests/native/r1_harness.hip):
libr1_harness.so under tests/_build/, compiled with build.py's compiler, target, flags
and include paths and stamped with a hash of the harness and of every file under csrc/
(as tests/sel_harness.py does), so that it is rebuilt only when one of them changed.
__graft_entry__.build() builds it with the rest; tests/test_gpu_r1_nodes.py loads it."""
from __future__ import annotations

import ctypes
import hashlib
import os
import subprocess

import numpy as np

from quantized_decoder_polar_codes_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "r1_harness.hip")
OUT_DIR = os.path.join(HERE, "_build")
LIB = os.path.join(OUT_DIR, "libr1_harness.so")
TAG = b"qpd-r1h-build-id:"

# r1_prep instantiations (enum Inst), rank sources (enum Src) and node modes (enum Mode)
GEN7, RK7, GEN15 = range(3)
SRC_RK, SRC_VUNI, SRC_TAB = range(3)
SMALL0, SMALL8, SMALL16, MULTI, MULTI_GEN = range(5)
MAXM = {GEN7: 7, RK7: 7, GEN15: 15}
ORD = 16  # order / symbol outputs per lane


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
        "-I", os.path.join(B.ROOT, "include"), "-I", B.SRC, f'-DQPD_R1_BUILD_ID="{source_hash()}"',
        "-shared", SRC, "-o", LIB + ".tmp"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    os.replace(LIB + ".tmp", LIB)
    return LIB


_F64 = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_I32 = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_U32 = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
_U16 = np.ctypeslib.ndpointer(np.uint16, flags="C_CONTIGUOUS")
_U8 = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")
_INT = ctypes.c_int


class Harness:
    def __init__(self, path: str):
        lib = ctypes.CDLL(path)
        lib.qpd_r1_build_id.restype = ctypes.c_char_p
        lib.qpd_r1_group_size.argtypes = [_INT]
        lib.qpd_r1_argsort.argtypes = [_INT] * 7 + [_U16, _U8, _I32, _I32, _U32, _I32]
        lib.qpd_r1_argsort_ref.argtypes = [_INT] * 5 + [_U16, _U8, _I32, _I32, _U32]
        lib.qpd_r1_heap.argtypes = [_INT, _INT, ctypes.c_int64, _I32, _U8, _I32]
        lib.qpd_r1_node.argtypes = [_INT] * 7 + [_F64, _F64, _U8, _U32, _F64, _I32, _I32]
        lib.qpd_r1_node_ref.argtypes = [_INT] * 5 + [_F64, _F64, _U8, _U32, _F64, _I32, _U32]
        self.lib = lib
        self.build_id = lib.qpd_r1_build_id().decode()

    def group_size(self, L: int) -> int:
        return int(self.lib.qpd_r1_group_size(L))

    # -- argsort -----------------------------------------------------------------------
    def argsort_raw(self, inst, src, L, temp, v, nsets, nblocks, table, sym):
        """The entry point's return code alone (argument validation)."""
        n = max(1, nblocks) * max(1, nsets) * 64
        out = [np.zeros(n * ORD, np.int32), np.zeros(n * ORD, np.int32), np.zeros(n, np.uint32),
               np.zeros(max(1, nblocks), np.int32)]
        return int(self.lib.qpd_r1_argsort(inst, src, L, temp, v, nsets, nblocks, np.ascontiguousarray(table, np.uint16),
                                           np.ascontiguousarray(sym, np.uint8), *out))

    def argsort(self, inst, src, L, v, table, sym):
        """table: uint16 [blocks, temp, v] rank << 1 | sign; sym: uint8 [blocks, sets, 64, temp].
        Returns ord, sym ([blocks, sets, 64, 16], -1 from m on), hw and the blocks' flags
        (bit 0 canaries intact, bit 1 source rows unchanged)."""
        table = np.ascontiguousarray(table, np.uint16)
        sym = np.ascontiguousarray(sym, np.uint8)
        nb, ns, _, temp = sym.shape
        assert sym.shape[2] == 64 and table.shape == (nb, temp, v), (sym.shape, table.shape)
        ord_ = np.empty((nb, ns, 64, ORD), np.int32)
        symo = np.empty((nb, ns, 64, ORD), np.int32)
        hw = np.empty((nb, ns, 64), np.uint32)
        ok = np.empty(nb, np.int32)
        rc = self.lib.qpd_r1_argsort(inst, src, L, temp, v, ns, nb, table, sym, ord_, symo, hw, ok)
        assert rc == 0, f"qpd_r1_argsort: error {rc}"
        return ord_, symo, hw, ok

    def argsort_ref(self, L, v, table, sym):
        table = np.ascontiguousarray(table, np.uint16)
        sym = np.ascontiguousarray(sym, np.uint8)
        nb, ns, _, temp = sym.shape
        ord_ = np.empty((nb, ns, 64, ORD), np.int32)
        symo = np.empty((nb, ns, 64, ORD), np.int32)
        hw = np.empty((nb, ns, 64), np.uint32)
        rc = self.lib.qpd_r1_argsort_ref(L, temp, v, ns, nb, table, sym, ord_, symo, hw)
        assert rc == 0, f"qpd_r1_argsort_ref: error {rc}"
        return ord_, symo, hw

    def heap(self, ranks, m):
        """ranks: int [..., temp].  Per array: does the introsort reach its depth limit (the
        heap-sort fallback) when the first m outputs are wanted, and the partitions it ran."""
        ranks = np.ascontiguousarray(ranks, np.int32)
        temp = ranks.shape[-1]
        n = ranks.size // temp
        fell, parts = np.empty(ranks.shape[:-1], np.uint8), np.empty(ranks.shape[:-1], np.int32)
        rc = self.lib.qpd_r1_heap(temp, m, n, ranks, fell, parts)
        assert rc == 0, f"qpd_r1_heap: error {rc}"
        return fell.astype(bool), parts

    # -- whole nodes ---------------------------------------------------------------------
    def node_raw(self, mode, src, L, temp, v, nsets, nblocks, quanta, pm, sym):
        n = max(1, nblocks) * max(1, nsets) * 64
        out = [np.zeros(n, np.uint32), np.zeros(n, np.float64), np.zeros(n, np.int32), np.zeros(max(1, nblocks), np.int32)]
        return int(self.lib.qpd_r1_node(mode, src, L, temp, v, nsets, nblocks, np.ascontiguousarray(quanta, np.float64),
                                        np.ascontiguousarray(pm, np.float64), np.ascontiguousarray(sym, np.uint8), *out))

    def node(self, mode, src, L, quanta, pm, sym):
        """quanta: [blocks, v]; pm: [blocks, sets, 64]; sym: uint8 [blocks, sets, 64, temp].
        Returns word, pm, lineage ([blocks, sets, 64]) and the blocks' flags."""
        quanta = np.ascontiguousarray(quanta, np.float64)
        pm = np.ascontiguousarray(pm, np.float64)
        sym = np.ascontiguousarray(sym, np.uint8)
        nb, ns, _, temp = sym.shape
        v = quanta.shape[1]
        assert pm.shape == (nb, ns, 64) and quanta.shape[0] == nb
        word, pmo, lin = np.empty(pm.shape, np.uint32), np.empty(pm.shape, np.float64), np.empty(pm.shape, np.int32)
        ok = np.empty(nb, np.int32)
        rc = self.lib.qpd_r1_node(mode, src, L, temp, v, ns, nb, quanta, pm, sym, word, pmo, lin, ok)
        assert rc == 0, f"qpd_r1_node: error {rc}"
        return word, pmo, lin, ok

    def node_ref(self, L, quanta, pm, sym):
        """The reference node; also ident ([blocks, sets, 64]): bit q = layer q's selection was
        the identity in the lane's group."""
        quanta = np.ascontiguousarray(quanta, np.float64)
        pm = np.ascontiguousarray(pm, np.float64)
        sym = np.ascontiguousarray(sym, np.uint8)
        nb, ns, _, temp = sym.shape
        word, pmo, lin = np.empty(pm.shape, np.uint32), np.empty(pm.shape, np.float64), np.empty(pm.shape, np.int32)
        ident = np.empty(pm.shape, np.uint32)
        rc = self.lib.qpd_r1_node_ref(L, temp, quanta.shape[1], ns, nb, quanta, pm, sym, word, pmo, lin, ident)
        assert rc == 0, f"qpd_r1_node_ref: error {rc}"
        return word, pmo, lin, ident


def load() -> Harness:
    h = Harness(build())
    if h.build_id != source_hash():
        raise RuntimeError(f"{LIB} carries build id {h.build_id}, the tree hashes to {source_hash()}")
    return h
