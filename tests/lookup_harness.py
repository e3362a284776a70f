"""Build and load helper of the lookup harness (tests/native/lookup_harness.hip): three
libraries under tests/_build/ from the one source -- liblookup_harness_chain0.so
(-DQPD_VEC_CHAIN=0), _chain1.so (-DQPD_VEC_CHAIN=1, as the FastSCL-LUT units compile lut_vec)
and _gswz72.so (-DQPD_GSWZ=72: the bank swizzle of the g table's u = 1 half) -- compiled with
build.py's compiler, target, flags and include paths and stamped with a hash of the harness,
of every file under csrc/ and of the variant's switches (as tests/r1_harness.py does), so that
each is rebuilt only when one of them changed.  __graft_entry__.build() builds them with the
rest; tests/test_gpu_lookup.py loads them."""
from __future__ import annotations

import ctypes
import hashlib
import os
import subprocess

import numpy as np

from quantized_decoder_polar_codes_amd import build as B

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "lookup_harness.hip")
OUT_DIR = os.path.join(HERE, "_build")
TAG = b"qpd-lkh-build-id:"
VARIANTS = {"chain0": ["-DQPD_VEC_CHAIN=0"], "chain1": ["-DQPD_VEC_CHAIN=1"], "gswz72": ["-DQPD_GSWZ=72"]}

# enum Fn, enum Chan, enum Kind of the harness
(LUT4, VEC2, VEC4, VEC8, VEC8IL, BYTE2, BYTE2H, BYTE4, BYTE4H, LDS8F, LDS8G, LDS8GIL, LDS8F512, INTERLEAVE, ILNIB, HALF2,
 HALF4, PACK4, N2B4, NIBMASK, POLAR) = range(21)
W8_I32_VEC, W8_I32, W8_U8_VEC, W8_U8, WORD_I32, WORD_U8, SMALL = range(7)
K_FG, K_FGP, K_CHAN, K_FF, K_GSEL = range(5)
T_F, T_G, T_FF = range(3)  # the table register row: f of node 0, g, both f tables
SRC_LDS, DST_LDS, U_LDS, CHILD_LDS = 1, 2, 4, 8  # `spaces` of an op


def lib_path(variant: str) -> str:
    return os.path.join(OUT_DIR, f"liblookup_harness_{variant}.so")


def source_hash(variant: str, extra=()) -> str:
    h = hashlib.sha256()
    h.update(repr((B.ARCH, B.COMMON_FLAGS, VARIANTS[variant], list(extra))).encode())
    for path in [SRC] + B._sources():
        h.update(os.path.relpath(path, B.ROOT).encode() + b"\0")
        with open(path, "rb") as f:
            h.update(f.read())
        h.update(b"\0")
    return h.hexdigest()[:32]


def library_build_id(path: str) -> str | None:
    try:
        with open(path, "rb") as f:
            data = f.read()
    except OSError:
        return None
    i = data.find(TAG)
    return None if i < 0 else data[i + len(TAG): i + len(TAG) + 32].decode("ascii", "replace")


def needs_build(variant: str) -> bool:
    return library_build_id(lib_path(variant)) != source_hash(variant)


def _command(variant: str, out: str, extra=()) -> list:
    return [B.HIPCC, f"--offload-arch={B.ARCH}"] + B.COMMON_FLAGS + VARIANTS[variant] + list(extra) + [
        "-I", os.path.join(B.ROOT, "include"), "-I", B.SRC, f'-DQPD_LK_BUILD_ID="{source_hash(variant, extra)}"',
        "-shared", SRC, "-o", out]


def build(force: bool = False, verbose: bool = False) -> dict:
    """Every variant (the stale ones compiled side by side); returns {variant: path}."""
    todo = [v for v in VARIANTS if force or needs_build(v)]
    os.makedirs(OUT_DIR, exist_ok=True)
    procs = []
    for v in todo:
        cmd = _command(v, lib_path(v) + ".tmp")
        if verbose:
            print(" ".join(cmd))
        procs.append((v, cmd, subprocess.Popen(cmd)))
    failed = [(v, cmd, p.returncode) for v, cmd, p in procs if p.wait() != 0]
    if failed:
        raise subprocess.CalledProcessError(failed[0][2], failed[0][1])
    for v in todo:
        os.replace(lib_path(v) + ".tmp", lib_path(v))
    return {v: lib_path(v) for v in VARIANTS}


_I32 = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
_U32 = np.ctypeslib.ndpointer(np.uint32, flags="C_CONTIGUOUS")
_U8 = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")
_INT = ctypes.c_int


def _tabs(tf, tg, v):
    tf = np.ascontiguousarray(tf, np.uint8)
    tg = np.ascontiguousarray(tg, np.uint8)
    assert tf.shape == (2, v, v) and tg.shape == (2, v, v), (tf.shape, tg.shape)
    return tf, tg


class Harness:
    def __init__(self, path: str):
        lib = ctypes.CDLL(path)
        lib.qpd_lk_build_id.restype = ctypes.c_char_p
        lib.qpd_lk_variant.argtypes = [ctypes.POINTER(ctypes.c_int32)] * 3
        lib.qpd_lk_variant.restype = None
        lib.qpd_lk_prim.argtypes = [_INT, _INT, _INT, _U8, _U8, _INT, _U32, _U32, _U32, _U32, _I32]
        lib.qpd_lk_chan.argtypes = [_INT, _INT, _INT, ctypes.c_int64, ctypes.c_void_p, _I32, _I32, _U32, _I32]
        lib.qpd_lk_op.argtypes = [_INT] * 11 + [_I32, _INT, _INT, _INT, _U8, _U8, _I32, _U32, _U32, _U8, _U8, _I32, _I32]
        lib.qpd_lk_root_pre.argtypes = [_INT, _INT, _INT, ctypes.c_int64, _INT, _INT, _INT, _U8, _U8, ctypes.c_void_p, _U32,
                                        _I32]
        self.lib = lib
        self.build_id = lib.qpd_lk_build_id().decode()
        sw = [ctypes.c_int32() for _ in range(3)]
        lib.qpd_lk_variant(*[ctypes.byref(x) for x in sw])
        self.vec_chain, self.gswz, self.lutmask = (int(x.value) for x in sw)

    def prim_raw(self, fn, tsel, v, tf, tg, a, b=None, h=None):
        """(return code, out, ok): n = a.size lanes (padded by the caller to a multiple of 64)."""
        tf, tg = _tabs(tf, tg, v)
        a = np.ascontiguousarray(a, np.uint32).reshape(-1)
        b = np.zeros_like(a) if b is None else np.ascontiguousarray(b, np.uint32).reshape(-1)
        h = np.zeros_like(a) if h is None else np.ascontiguousarray(h, np.uint32).reshape(-1)
        out, ok = np.zeros(a.size, np.uint32), np.zeros(max(1, a.size // 64), np.int32)
        return int(self.lib.qpd_lk_prim(fn, tsel, v, tf, tg, a.size, a, b, h, out, ok)), out, ok

    def prim(self, fn, tsel, v, tf, tg, a, b=None, h=None):
        """The function on every lane of a (any length: padded with copies of lane 0).  Asserts the
        blocks' canaries."""
        a = np.asarray(a, np.uint32).reshape(-1)
        n = a.size
        pad = (-n) % 64

        def padded(x):
            if x is None:
                return None
            x = np.asarray(x, np.uint32).reshape(-1)
            return np.concatenate([x, np.repeat(x[:1], pad)])

        rc, out, ok = self.prim_raw(fn, tsel, v, tf, tg, padded(a), padded(b), padded(h))
        assert rc == 0, f"qpd_lk_prim({fn}): error {rc}"
        assert (ok == 3).all(), f"qpd_lk_prim({fn}): canaries of blocks {np.flatnonzero(ok != 3)[:8]}"
        return out[:n]

    def chan_raw(self, mode, v, buf, e0, cnt):
        buf = np.ascontiguousarray(buf)
        assert buf.dtype in (np.int32, np.uint8)
        e0 = np.ascontiguousarray(e0, np.int32).reshape(-1)
        cnt = np.ascontiguousarray(cnt, np.int32).reshape(-1)
        out, err = np.zeros(e0.size, np.uint32), np.zeros(e0.size, np.int32)
        rc = self.lib.qpd_lk_chan(mode, v, e0.size, buf.size, buf.ctypes.data_as(ctypes.c_void_p), e0, cnt, out, err)
        return int(rc), out, err

    def chan(self, mode, v, buf, e0, cnt):
        """Reader `mode` once per lane (e0.size a multiple of 64): (word, error word) per lane."""
        rc, out, err = self.chan_raw(mode, v, buf, e0, cnt)
        assert rc == 0, f"qpd_lk_chan({mode}): error {rc}"
        return out, err

    def op_raw(self, kind, isg, lt, pre, cnt, v, in_vec, gs, spaces, rows, tf, tg, y, lds, slab, srcf, usrcf):
        """lds / slab: uint32 [blocks, rows, sets, 64]; y: int32 [blocks, sets, 64 // gs, ystride];
        srcf / usrcf: uint8 [blocks, sets, 64].  Returns (rc, lds, slab, err, ok) after the op."""
        tf, tg = _tabs(tf, tg, v)
        lds = np.array(lds, np.uint32, order="C")
        slab = np.array(slab, np.uint32, order="C")
        y = np.ascontiguousarray(y, np.int32)
        srcf = np.ascontiguousarray(srcf, np.uint8)
        usrcf = np.ascontiguousarray(usrcf, np.uint8)
        nb, lds_rows, ns, _ = lds.shape
        assert slab.shape[0] == nb and slab.shape[2:] == (ns, 64) and lds.shape[3] == 64
        assert y.shape[:3] == (nb, ns, 64 // gs) and srcf.shape == usrcf.shape == (nb, ns, 64)
        err, ok = np.zeros(nb, np.int32), np.zeros(nb, np.int32)
        rc = self.lib.qpd_lk_op(kind, int(isg), int(lt), int(pre), cnt, v, int(in_vec), gs, ns, nb, spaces,
                                np.ascontiguousarray(rows, np.int32), lds_rows, slab.shape[1], y.shape[3], tf, tg, y, lds, slab,
                                srcf, usrcf, err, ok)
        return int(rc), lds, slab, err, ok

    def root_pre_raw(self, u8, n, v, grid, in_vec, in_off, tf, tg, inp, pre):
        """inp: int32 / uint8 [in_off + B * N]; pre: uint32 [(B + 1) * N / 4] sentinels.  (rc, pre, err)."""
        tf, tg = _tabs(tf, tg, v)
        inp = np.ascontiguousarray(inp, np.uint8 if u8 else np.int32)
        pre = np.array(pre, np.uint32, order="C").reshape(-1)
        B_ = (inp.size - in_off) >> n
        err = np.zeros(1, np.int32)
        rc = self.lib.qpd_lk_root_pre(int(u8), n, v, B_, grid, int(in_vec), in_off, tf, tg,
                                      inp.ctypes.data_as(ctypes.c_void_p), pre, err)
        return int(rc), pre, int(err[0])


def load(variant: str = "chain0") -> Harness:
    h = Harness(build()[variant])
    if h.build_id != source_hash(variant):
        raise RuntimeError(f"{lib_path(variant)} carries build id {h.build_id}, the tree hashes to {source_hash(variant)}")
    return h

