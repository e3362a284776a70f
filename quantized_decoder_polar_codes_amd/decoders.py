"""Host-side mirror of the reference's pybind11 decoder classes -- all 15 of
_libPolarDecoder.cpp:29-50.

Same class names, positional order, keyword names and ``decode`` argument as
the reference (py_interface/py_SCLUTDecoder.cpp:11-14, py_SCLLUTDecoder.cpp:12-15,
py_FastSCLUTDecoder.cpp:12-15, py_FastSCLLUTDecoder.cpp:13-16,
py_SCDecoder.cpp:10-12, py_SCLDecoder.cpp:10-12, py_CASCLDecoder.cpp:10-13,
py_FastSCDecoder.cpp:11-14, py_FastSCLDecoder.cpp:10-13,
py_SCUniformDecoder.cpp:10-14, py_SCLUniformQuantizedDecoder.cpp:10-14,
py_SCLloydQuantizedDecoder.cpp:10-15, py_SCLLloydQuantizedDecoder.cpp:10-15):
``decode`` takes one frame and returns a new ``numpy.ndarray`` of dtype uint8
and length K (A for the CRC-aided classes).  Every decode runs in libqpd.so:
batches on the GPU kernels, the few frames of a per-frame call on its host
engine (qpd_decode_host; a GPU call costs ~0.1 ms before decoding anything,
the reference's SC-LUT call ~10 us).  The package fails to load without the
library and a decoder cannot be created without a HIP device.

Additions (not in the reference): ``decode_batch(x[B, N])`` for throughput
(numpy in -> numpy out; a torch CUDA tensor in -> torch CUDA tensor out,
asynchronous on torch's current stream), and validation with ``ValueError``
where the reference has undefined behaviour.
"""
from __future__ import annotations

import ctypes
import threading
from typing import NamedTuple

import numpy as np

from . import _lib
from .lut import PackedLUT, pack_luts
from .quant import LloydQuant, UniformQuant, pack_lloyd, pack_uniform

__all__ = ["ChannelQuantizer", "DecodeStatus", "DecodeList", "MaskSearch", "SCDecoder", "SCLUTDecoder", "SCLLUTDecoder", "FastSCLUTDecoder", "FastSCLLUTDecoder",
           "CASCLLUTDecoder", "CAFastSCLLUTDecoder", "SCLDecoder", "CASCLDecoder", "FastSCDecoder", "FastSCLDecoder",
           "SCUniformQuantizedDecoder", "SCLUniformQuantizedDecoder", "SCLloydQuantizedDecoder",
           "SCLLloydQuantizedDecoder"]

# The CRC the reference CA decoders actually check (CASCLLUTDecoder.h:33-34,
# CAFastSCLLUTDecoder.h:29-30): CRC-24 with these coefficient indices, whatever
# crc_n / crc_p the CASCLLUTDecoder constructor receives (decode never reads them).
CRC24_LOC = (24, 23, 21, 20, 17, 15, 13, 12, 8, 4, 2, 1, 0)


def _as_i32(x) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x).astype(np.int32))


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


class DecodeStatus(NamedTuple):
    """What ``decode_batch(..., return_status=True)`` returns beside the bits, per frame:
    ``metric`` (float64 [B]), the path metric of the output path, and ``crc_pass`` (bool [B];
    None for a decoder without CRC), whether that path passed the CRC compare
    (qpd_decode_status, include/qpd.h).  numpy arrays or torch CUDA tensors, as the bits."""

    metric: object
    crc_pass: object


class DecodeList(NamedTuple):
    """What ``decode_list_batch`` returns: all L candidates of every frame in the reference's
    argsort order of the path metrics (qpd_decode_list, include/qpd.h) -- ``bits`` (uint8
    [B, L, K]), ``metric`` (float64 [B, L]), ``crc_pass`` (bool [B, L]; None for a decoder
    without CRC), ``chosen`` (int32 [B]: the candidate whose bits are output) and ``out`` (uint8
    [B, out_bits], ``decode_batch``'s bits).  numpy arrays or torch CUDA tensors."""

    bits: object
    metric: object
    crc_pass: object
    chosen: object
    out: object


class MaskSearch(NamedTuple):
    """What ``decode_search_batch`` returns (qpd_decode_search, include/qpd.h): ``out`` (uint8
    [B, A], the output path's bits), ``hit_mask`` (int32 [B]: the index of the mask that passed,
    -1: none), ``hit_rank`` (int32 [B]: the output path's rank in the argsort of the path
    metrics), ``metric`` (float64 [B], its metric), ``syndrome`` (uint32 [B, L]: every
    candidate's CRC syndrome) and ``cand_metric`` (float64 [B, L]).  The first four are None for
    an empty mask set.  numpy arrays or torch CUDA tensors."""

    out: object
    hit_mask: object
    hit_rank: object
    metric: object
    syndrome: object
    cand_metric: object


def _torch():
    try:
        import torch  # noqa: F401

        return torch
    except Exception:  # pragma: no cover - torch is part of the image
        return None


class ChannelQuantizer:
    """The drivers' channel quantizer as a value (mainQuantizedDecoder_LLRDomain.py:135-145,
    :167-176): ``edges`` (interval_x, ascending, 2..257 of them), ``lut`` (channel_lut, one entry in
    [0, q) per bin) and ``q`` channel symbols -- what ``lutgen.channel_quantizer`` (its
    interval_x and channel_lut), ``lutgen.design`` (the same call at the design's sigma) and
    ``montecarlo.uniform_channel_quantizer`` return.  Validated once; keeps the arrays the C
    struct points to alive.  ``decode_llr_batch`` / ``quantize_llr`` of the LUT decoders take it."""

    def __init__(self, edges, lut, q: int | None = None):
        self.edges = np.ascontiguousarray(np.asarray(edges, dtype=np.float64).reshape(-1))
        lut = np.asarray(lut).reshape(-1)
        self.lut = np.ascontiguousarray(lut.astype(np.int32))
        if not 2 <= self.edges.size <= 257:
            raise ValueError(f"a channel quantizer has 2..257 edges, got {self.edges.size}")
        if self.lut.size != self.edges.size - 1 or not (self.lut == lut).all():
            raise ValueError(f"lut must have one integer per bin ({self.edges.size - 1}), got {lut.size} entries")
        if not (self.edges[:-1] <= self.edges[1:]).all():  # a NaN edge fails it too
            raise ValueError("edges must be ascending")
        self.q = int(self.lut.max()) + 1 if q is None else int(q)
        if self.q < 2 or self.lut.min() < 0 or self.lut.max() >= self.q:
            raise ValueError(f"lut entries must be in [0, q) with q >= 2 (q = {self.q})")
        self.ch = _lib.QpdMcChannel()
        self.ch.sigma = 0.0  # not read by the LLR entry points
        self.ch.q, self.ch.n_edges = self.q, self.edges.size
        self.ch.edges, self.ch.lut = self.edges.ctypes.data, self.lut.ctypes.data

    @classmethod
    def uniform(cls, v: int = 16, delta: float = 0.5):
        """montecarlo.uniform_channel_quantizer(v, delta)."""
        from .montecarlo import uniform_channel_quantizer

        return cls(*uniform_channel_quantizer(v, delta), q=v)

    @classmethod
    def mindistortion(cls, sigma: float, q_uniform: int = 128, q: int = 16, sum_order: str = "cpp"):
        """lutgen.channel_quantizer(sigma, q_uniform, q): the drivers' design for AWGN std sigma."""
        from .lutgen import channel_quantizer

        _, _, edges, lut = channel_quantizer(sigma, q_uniform, q, sum_order)
        return cls(edges, lut, q=q)

    @classmethod
    def for_design(cls, design, q_uniform: int = 128, sum_order: str = "cpp"):
        """The channel quantizer a ``lutgen.design`` result was designed with (its design SNR and v)."""
        return cls.mindistortion(float(np.sqrt(1 / 10 ** (design.design_snr_db / 10))), q_uniform, design.v, sum_order)

    def __call__(self, llr) -> np.ndarray:
        """The symbols on the host (codes.quantize_channel)."""
        from .codes import quantize_channel

        return quantize_channel(llr, self.edges, self.lut, self.q)


class _DecoderBase:
    _kind: int = -1

    @property
    def _float_input(self) -> bool:
        return self._kind in _lib.FLOAT_KINDS

    def __init__(self, N, K, L, frozen_bits, message_bits, node_type, packed: PackedLUT | None, device=None,
                 max_waves: int = 0, engine: str = "auto", A: int | None = None, crc_n: int = 24,
                 crc_loc=CRC24_LOC, quant: UniformQuant | LloydQuant | None = None, create: bool = True):
        self.N = int(N)
        self.K = int(K)
        self.L = int(L)
        self.A = self.K if A is None else int(A)
        self.out_bits = self.A
        frozen = _as_i32(frozen_bits).reshape(-1)
        if frozen.size != self.N:
            raise ValueError(f"frozen_bits must have N={self.N} entries, got {frozen.size}")
        self.frozen_bits = frozen
        # message_bits is stored but never read by the reference
        self.message_bits = np.asarray(message_bits)
        self.node_type = None if node_type is None else _as_i32(node_type).reshape(-1)
        if self.node_type is not None and self.node_type.size != 2 * self.N - 1:
            raise ValueError(f"node_type must have 2N-1={2 * self.N - 1} entries, got {self.node_type.size}")
        self.packed = packed
        cfg = _lib.QpdConfig()
        cfg.kind = self._kind
        cfg.N, cfg.K, cfg.L = self.N, self.K, self.L
        cfg.frozen_bits = _ptr(self.frozen_bits)
        cfg.node_type = _ptr(self.node_type)
        if packed is not None:
            if packed.N != self.N:
                raise ValueError(f"tables are for N={packed.N}, decoder N={self.N}")
            cfg.v = packed.v
            cfg.lut_f, cfg.lut_f_count = _ptr(packed.lut_f), packed.lut_f.shape[0]
            cfg.f_base, cfg.f_step = _ptr(packed.f_base), packed.f_step
            cfg.lut_g, cfg.lut_g_count = _ptr(packed.lut_g), packed.lut_g.shape[0]
            cfg.g_base, cfg.g_step = _ptr(packed.g_base), packed.g_step
            cfg.vcl, cfg.vcl_rows = _ptr(packed.vcl), packed.vcl_rows
        if device is None:
            torch = _torch()
            device = torch.cuda.current_device() if torch is not None and torch.cuda.is_available() else -1
        self.device = int(device)
        cfg.device = self.device
        cfg.max_waves = int(max_waves)
        cfg.engine = {"auto": _lib.QPD_ENGINE_AUTO, "generic": _lib.QPD_ENGINE_GENERIC,
                      "fast": _lib.QPD_ENGINE_FAST}[engine]
        self.quant = quant
        if isinstance(quant, UniformQuant):
            cfg.v = quant.v
            cfg.r_f, cfg.r_g = _ptr(quant.r_f), _ptr(quant.r_g)
        elif isinstance(quant, LloydQuant):
            cfg.v = quant.v
            cfg.q_bnd, cfg.q_bnd_count = _ptr(quant.bnd), quant.bnd.size
            cfg.q_rec, cfg.q_rec_count = _ptr(quant.rec), quant.rec.size
            cfg.bnd_off, cfg.bnd_len = _ptr(quant.bnd_off), _ptr(quant.bnd_len)
            cfg.rec_off, cfg.rec_len = _ptr(quant.rec_off), _ptr(quant.rec_len)
        self._crc_loc = np.ascontiguousarray(np.asarray(crc_loc, dtype=np.int32))
        if self._kind in (_lib.QPD_CASCL_LUT, _lib.QPD_CAFASTSCL_LUT, _lib.QPD_CASCL_FLOAT):
            cfg.A, cfg.crc_n = self.A, int(crc_n)
            cfg.crc_loc, cfg.crc_loc_count = _ptr(self._crc_loc), self._crc_loc.size
        self._cfg = cfg  # the arrays it points to are attributes of self
        if not create:  # configuration only (tests of the host engine on CPU): no device decoder
            self._h = None
            return
        h = ctypes.c_void_p()
        lib = _lib.load()
        _lib.check(lib.qpd_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h
        # the per-frame call's own buffers and bound entry point (numpy's
        # pointer extraction costs ~2 us per array, as much as a whole SC-LUT
        # frame on the host engine): decode() copies into / out of them
        self._one_in = np.empty(self.N, dtype=np.float64 if self._float_input else np.int32)
        self._one_out = np.empty(self.out_bits, dtype=np.uint8)
        self._one_args = (ctypes.c_void_p(self._one_in.ctypes.data), ctypes.c_void_p(self._one_out.ctypes.data))
        self._one_fn = lib.qpd_decode_f64_host if self._float_input else lib.qpd_decode_host
        self._one_lock = threading.Lock()

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                _lib.load().qpd_destroy(h)
            except Exception:
                pass
            self._h = None

    # -- introspection ---------------------------------------------------------
    def info(self) -> dict:
        inf = _lib.QpdInfo()
        _lib.check(_lib.load().qpd_get_info(self._h, ctypes.byref(inf)))
        return {k: getattr(inf, k) for k, _ in inf._fields_}

    def profile(self, enable: bool = True) -> None:
        """Bracket every kernel launch of this decoder with HIP events on its
        stream (qpd_profile); read the sums with :meth:`kernel_times`."""
        _lib.check(_lib.load().qpd_profile(self._h, int(bool(enable))))

    def kernel_times(self) -> dict:
        """{class: (ms summed, launches)} since the last call, for the classes
        'pre' (root pre-pass, or the LLR calls' quantizer), 'decode', 'mc' (frame generator) and 'pfx'
        (frozen prefix, lut_prefix_kernel)."""
        ms = (ctypes.c_double * _lib.QPD_KC_COUNT)()
        n = (ctypes.c_int64 * _lib.QPD_KC_COUNT)()
        _lib.check(_lib.load().qpd_kernel_times(self._h, ms, n))
        return {name: (ms[i], n[i]) for i, name in enumerate(("pre", "decode", "mc", "pfx"))}

    # -- decoding --------------------------------------------------------------
    @property
    def _crc_aided(self) -> bool:
        return self._kind in (_lib.QPD_CASCL_LUT, _lib.QPD_CAFASTSCL_LUT, _lib.QPD_CASCL_FLOAT)

    def _decode_status(self, x, crc_mask):
        """decode_batch(x, return_status=True, crc_mask): qpd_decode_status / _host."""
        torch = _torch()
        lib = _lib.load()
        mask = None
        sa = _lib.QpdStatusArgs()
        if crc_mask is not None:
            mask = np.ascontiguousarray(np.asarray(crc_mask).reshape(-1).astype(np.uint8))
            sa.crc_mask, sa.crc_mask_bits = _ptr(mask), mask.size
        if torch is not None and isinstance(x, torch.Tensor) and x.is_cuda:
            u8 = not self._float_input and x.dtype == torch.uint8
            want = torch.float64 if self._float_input else torch.uint8 if u8 else torch.int32
            xs = x.reshape(-1, self.N).to(want).contiguous()
            B = xs.shape[0]
            out = torch.empty((B, self.out_bits), dtype=torch.uint8, device=xs.device)
            metric = torch.empty(B, dtype=torch.float64, device=xs.device)
            flag = torch.empty(B, dtype=torch.uint8, device=xs.device) if self._crc_aided else None
            sa.metric = ctypes.c_void_p(metric.data_ptr())
            sa.crc_pass = None if flag is None else ctypes.c_void_p(flag.data_ptr())
            ty = _lib.QPD_IN_F64 if self._float_input else _lib.QPD_IN_U8 if u8 else _lib.QPD_IN_I32
            stream = torch.cuda.current_stream(xs.device).cuda_stream
            _lib.check(lib.qpd_decode_status(self._h, ctypes.c_void_p(xs.data_ptr()), ty, B,
                                             ctypes.c_void_p(out.data_ptr()), ctypes.byref(sa), ctypes.c_void_p(stream)))
            return out, DecodeStatus(metric, None if flag is None else flag.bool())
        if torch is not None and isinstance(x, torch.Tensor):
            x = x.numpy()
        a = np.asarray(x)
        u8 = not self._float_input and a.dtype == np.uint8
        want = np.float64 if self._float_input else np.uint8 if u8 else np.int32
        a = np.ascontiguousarray(a.astype(want, copy=False).reshape(-1, self.N))
        B = a.shape[0]
        out = np.empty((B, self.out_bits), dtype=np.uint8)
        metric = np.zeros(B, dtype=np.float64)
        flag = np.zeros(B, dtype=np.uint8) if self._crc_aided else None
        sa.metric, sa.crc_pass = _ptr(metric), _ptr(flag)
        ty = _lib.QPD_IN_F64 if self._float_input else _lib.QPD_IN_U8 if u8 else _lib.QPD_IN_I32
        _lib.check(lib.qpd_decode_status_host(self._h, _ptr(a), ty, B, _ptr(out), ctypes.byref(sa)))
        return out, DecodeStatus(metric, None if flag is None else flag.astype(bool))

    def decode_list_batch(self, x, crc_mask=None):
        """All L candidates of a list decode (qpd_decode_list / _host) -> :class:`DecodeList`:
        ``bits [B, L, K]`` (for the CRC-aided decoders message and CRC tail), ``metric [B, L]``,
        ``crc_pass [B, L]`` (None without CRC), ``chosen [B]`` and ``out [B, out_bits]``, the
        bits of ``decode_batch``.  Candidate r is the path at position r of the reference's
        argsort of the path metrics (ascending, ties by list slot); ``chosen`` is the r whose
        bits ``out`` holds.  ``crc_mask`` as for ``decode_batch(return_status=True)``.  numpy in
        -> numpy out (synchronous); a torch CUDA tensor is read where it lies, on the current
        stream -> torch CUDA tensors.  List decoders with 2 <= L <= 16."""
        torch = _torch()
        lib = _lib.load()
        mask = None
        la = _lib.QpdListArgs()
        if crc_mask is not None:
            mask = np.ascontiguousarray(np.asarray(crc_mask).reshape(-1).astype(np.uint8))
            la.crc_mask, la.crc_mask_bits = _ptr(mask), mask.size
        ca, L, K = self._crc_aided, int(self.L), int(self.K)
        if torch is not None and isinstance(x, torch.Tensor) and x.is_cuda:
            u8 = not self._float_input and x.dtype == torch.uint8
            want = torch.float64 if self._float_input else torch.uint8 if u8 else torch.int32
            xs = x.reshape(-1, self.N).to(want).contiguous()
            B = xs.shape[0]
            dev = xs.device
            out = torch.empty((B, self.out_bits), dtype=torch.uint8, device=dev)
            bits = torch.empty((B, L, K), dtype=torch.uint8, device=dev)
            metric = torch.empty((B, L), dtype=torch.float64, device=dev)
            flag = torch.empty((B, L), dtype=torch.uint8, device=dev) if ca else None
            chosen = torch.empty(B, dtype=torch.int32, device=dev)
            la.cand_bits = ctypes.c_void_p(bits.data_ptr())
            la.cand_metric = ctypes.c_void_p(metric.data_ptr())
            la.cand_pass = None if flag is None else ctypes.c_void_p(flag.data_ptr())
            la.chosen = ctypes.c_void_p(chosen.data_ptr())
            ty = _lib.QPD_IN_F64 if self._float_input else _lib.QPD_IN_U8 if u8 else _lib.QPD_IN_I32
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.qpd_decode_list(self._h, ctypes.c_void_p(xs.data_ptr()), ty, B,
                                           ctypes.c_void_p(out.data_ptr()), ctypes.byref(la), ctypes.c_void_p(stream)))
            return DecodeList(bits, metric, None if flag is None else flag.bool(), chosen, out)
        if torch is not None and isinstance(x, torch.Tensor):
            x = x.numpy()
        a = np.asarray(x)
        u8 = not self._float_input and a.dtype == np.uint8
        want = np.float64 if self._float_input else np.uint8 if u8 else np.int32
        a = np.ascontiguousarray(a.astype(want, copy=False).reshape(-1, self.N))
        B = a.shape[0]
        out = np.zeros((B, self.out_bits), dtype=np.uint8)
        bits = np.zeros((B, L, K), dtype=np.uint8)
        metric = np.zeros((B, L), dtype=np.float64)
        flag = np.zeros((B, L), dtype=np.uint8) if ca else None
        chosen = np.zeros(B, dtype=np.int32)
        la.cand_bits, la.cand_metric, la.cand_pass, la.chosen = _ptr(bits), _ptr(metric), _ptr(flag), _ptr(chosen)
        ty = _lib.QPD_IN_F64 if self._float_input else _lib.QPD_IN_U8 if u8 else _lib.QPD_IN_I32
        _lib.check(lib.qpd_decode_list_host(self._h, _ptr(a), ty, B, _ptr(out), ctypes.byref(la)))
        return DecodeList(bits, metric, None if flag is None else flag.astype(bool), chosen, out)

    @staticmethod
    def _mask_set(crc_masks, mask_bits):
        """``crc_masks`` of ``decode_search_batch`` as a uint8 [R, bits] array of 0/1 rows."""
        a = np.asarray(crc_masks)
        if a.ndim == 2:
            if mask_bits is not None and int(mask_bits) != a.shape[1]:
                raise ValueError(f"crc_masks has rows of {a.shape[1]} bits, mask_bits = {mask_bits}")
            if a.size and not ((a == 0) | (a == 1)).all():  # before the cast: 256 or 2.7 would become valid entries
                raise ValueError("crc_masks entries must be 0 or 1")
            return np.ascontiguousarray(a.astype(np.uint8))
        bits = 16 if mask_bits is None else int(mask_bits)
        if not 0 <= bits <= 32:
            raise ValueError(f"mask_bits must be in [0, 32], got {bits}")
        vals = [int(m) for m in a.reshape(-1)]
        if any(m < 0 or m >> bits for m in vals):
            raise ValueError(f"a mask does not fit {bits} bits")
        rows = [[(m >> (bits - 1 - l)) & 1 for l in range(bits)] for m in vals]  # most significant bit first
        return np.ascontiguousarray(np.array(rows, dtype=np.uint8).reshape(len(vals), bits))

    def decode_search_batch(self, x, crc_masks, mask_bits=None):
        """One list decode against a set of CRC masks (qpd_decode_search / _host) ->
        :class:`MaskSearch`: which of the masks (e.g. the RNTIs a receiver holds), if any, a
        frame is addressed to, and on which list path.  ``crc_masks``: an ``[R, bits]`` array
        of 0/1 rows (each as ``crc_mask`` of ``decode_batch``), or a sequence of R ints of
        ``mask_bits`` bits (default 16), most significant bit first; R <= 256.  The output path
        is the lowest rank ``hit_rank`` (position in the argsort of the path metrics) that any
        mask passes, ``hit_mask`` the lowest index that passes it (-1: none did, the output is
        the best-metric path); ``out [B, A]`` and ``metric [B]`` are that path's.  ``syndrome
        [B, L]`` (uint32) is every candidate's CRC syndrome -- the mask that would pass it,
        cut to the compared bits -- and ``cand_metric [B, L]`` its metric.  An empty
        ``crc_masks``: the syndromes and metrics alone (the other fields None).  numpy in ->
        numpy out (synchronous); a torch CUDA tensor is read where it lies, on the current
        stream -> torch CUDA tensors.  CRC-aided decoders with 2 <= L <= 16."""
        torch = _torch()
        lib = _lib.load()
        masks = self._mask_set(crc_masks, mask_bits)
        R = masks.shape[0]
        sa = _lib.QpdSearchArgs()
        sa.crc_masks, sa.n_masks, sa.crc_mask_bits = (_ptr(masks) if masks.size else None), R, masks.shape[1]
        L = int(self.L)
        if torch is not None and isinstance(x, torch.Tensor) and x.is_cuda:
            u8 = not self._float_input and x.dtype == torch.uint8
            want = torch.float64 if self._float_input else torch.uint8 if u8 else torch.int32
            xs = x.reshape(-1, self.N).to(want).contiguous()
            B = xs.shape[0]
            dev = xs.device
            syn = torch.empty((B, L), dtype=torch.int32, device=dev)  # (torch has no uint32 arithmetic: a view below)
            cmet = torch.empty((B, L), dtype=torch.float64, device=dev)
            out = hit = rank = metric = None
            if R:
                out = torch.empty((B, self.out_bits), dtype=torch.uint8, device=dev)
                hit = torch.empty(B, dtype=torch.int32, device=dev)
                rank = torch.empty(B, dtype=torch.int32, device=dev)
                metric = torch.empty(B, dtype=torch.float64, device=dev)
            p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
            sa.cand_syndrome, sa.cand_metric = p(syn), p(cmet)
            sa.hit_mask, sa.hit_rank, sa.metric = p(hit), p(rank), p(metric)
            ty = _lib.QPD_IN_F64 if self._float_input else _lib.QPD_IN_U8 if u8 else _lib.QPD_IN_I32
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(lib.qpd_decode_search(self._h, ctypes.c_void_p(xs.data_ptr()), ty, B, p(out), ctypes.byref(sa),
                                             ctypes.c_void_p(stream)))
            return MaskSearch(out, hit, rank, metric, syn.view(torch.uint32), cmet)
        if torch is not None and isinstance(x, torch.Tensor):
            x = x.numpy()
        a = np.asarray(x)
        u8 = not self._float_input and a.dtype == np.uint8
        want = np.float64 if self._float_input else np.uint8 if u8 else np.int32
        a = np.ascontiguousarray(a.astype(want, copy=False).reshape(-1, self.N))
        B = a.shape[0]
        syn = np.zeros((B, L), dtype=np.uint32)
        cmet = np.zeros((B, L), dtype=np.float64)
        out = hit = rank = metric = None
        if R:
            out = np.zeros((B, self.out_bits), dtype=np.uint8)
            hit = np.zeros(B, dtype=np.int32)
            rank = np.zeros(B, dtype=np.int32)
            metric = np.zeros(B, dtype=np.float64)
        sa.cand_syndrome, sa.cand_metric = _ptr(syn), _ptr(cmet)
        sa.hit_mask, sa.hit_rank, sa.metric = _ptr(hit), _ptr(rank), _ptr(metric)
        ty = _lib.QPD_IN_F64 if self._float_input else _lib.QPD_IN_U8 if u8 else _lib.QPD_IN_I32
        _lib.check(lib.qpd_decode_search_host(self._h, _ptr(a), ty, B, _ptr(out), ctypes.byref(sa)))
        return MaskSearch(out, hit, rank, metric, syn, cmet)

    def decode_batch(self, x, return_status: bool = False, crc_mask=None):
        """Decode B frames.  numpy [B, N] -> numpy uint8 [B, K] (synchronous);
        torch CUDA tensor [B, N] -> torch CUDA uint8 [B, K] on the current stream.
        (A instead of K for the CRC-aided decoders.)  LUT decoders: uint8 symbols
        go to the library as they are (qpd_decode_u8 / qpd_decode_u8_host, a
        quarter of the bytes); any other dtype is converted to int32.
        ``return_status=True`` (list decoders): ``(bits, DecodeStatus)`` -- the output
        path's metric and, for the CRC-aided decoders, whether it passed the CRC;
        ``crc_mask`` (0/1 entries, at most crc_n; with return_status): XORed onto the tail
        of the computed CRC before the compare, e.g. the RNTI of a blind detection."""
        if return_status:
            return self._decode_status(x, crc_mask)
        if crc_mask is not None:
            raise ValueError("crc_mask needs return_status=True")
        torch = _torch()
        lib = _lib.load()
        if torch is not None and isinstance(x, torch.Tensor) and x.is_cuda:
            # uint8 symbols of a LUT decoder go to the library as they are (qpd_decode_u8);
            # every other dtype (int8 and bool included) is converted to int32 as before
            u8 = not self._float_input and x.dtype == torch.uint8
            want = torch.float64 if self._float_input else torch.uint8 if u8 else torch.int32
            xs = x.reshape(-1, self.N).to(want).contiguous()
            B = xs.shape[0]
            out = torch.empty((B, self.out_bits), dtype=torch.uint8, device=xs.device)
            stream = torch.cuda.current_stream(xs.device).cuda_stream
            fn = lib.qpd_decode_f64 if self._float_input else lib.qpd_decode_u8 if u8 else lib.qpd_decode
            _lib.check(fn(self._h, ctypes.c_void_p(xs.data_ptr()), B, ctypes.c_void_p(out.data_ptr()),
                          ctypes.c_void_p(stream)))
            return out
        if torch is not None and isinstance(x, torch.Tensor):
            x = x.numpy()
        a = np.asarray(x)
        u8 = not self._float_input and a.dtype == np.uint8
        want = np.float64 if self._float_input else np.uint8 if u8 else np.int32
        a = np.ascontiguousarray(a.astype(want, copy=False).reshape(-1, self.N))
        B = a.shape[0]
        out = np.empty((B, self.out_bits), dtype=np.uint8)
        fn = lib.qpd_decode_f64_host if self._float_input else lib.qpd_decode_u8_host if u8 else lib.qpd_decode_host
        _lib.check(fn(self._h, _ptr(a), B, _ptr(out)))
        return out

    # -- blind-detection metric --------------------------------------------------
    def dmetric_batch(self, llr, return_bits: bool = False):
        """The blind-detection metric of B frames of LLRs: the reference's
        ``DMetricCalculator.calculate`` (PolarBD, DMetric.cpp:24-177), batched -- the same
        double per frame.  ``FastSCDecoder`` only (the metric is its traversal's; the decoder's
        frozen_bits and node_type are the calculator's); every other class raises TypeError.
        A torch CUDA float64 tensor [B, N] is read where it is (qpd_dmetric on the current
        stream, no copy) -> torch CUDA float64 [B]; a numpy array or CPU tensor goes to
        qpd_dmetric_host -> numpy float64 [B]; other dtypes are converted to float64 as
        decode_batch converts them.  ``return_bits=True``: ``(metric, bits)``, bits as
        ``decode_batch(llr)``."""
        if self._kind != _lib.QPD_FASTSC_FLOAT:
            raise TypeError(f"dmetric_batch is FastSCDecoder's (the metric is the float FastSC traversal's), "
                            f"not {type(self).__name__}'s")
        torch = _torch()
        lib = _lib.load()
        if torch is not None and isinstance(llr, torch.Tensor) and llr.is_cuda:
            xs = llr.reshape(-1, self.N).to(torch.float64).contiguous()
            B = xs.shape[0]
            metric = torch.empty(B, dtype=torch.float64, device=xs.device)
            bits = torch.empty((B, self.out_bits), dtype=torch.uint8, device=xs.device) if return_bits else None
            stream = torch.cuda.current_stream(xs.device).cuda_stream
            _lib.check(lib.qpd_dmetric(self._h, ctypes.c_void_p(xs.data_ptr()), B, ctypes.c_void_p(metric.data_ptr()),
                                       None if bits is None else ctypes.c_void_p(bits.data_ptr()),
                                       ctypes.c_void_p(stream)))
            return (metric, bits) if return_bits else metric
        if torch is not None and isinstance(llr, torch.Tensor):
            llr = llr.numpy()
        a = np.ascontiguousarray(np.asarray(llr).astype(np.float64, copy=False).reshape(-1, self.N))
        B = a.shape[0]
        metric = np.empty(B, dtype=np.float64)
        bits = np.empty((B, self.out_bits), dtype=np.uint8) if return_bits else None
        _lib.check(lib.qpd_dmetric_host(self._h, _ptr(a), B, _ptr(metric), _ptr(bits)))
        return (metric, bits) if return_bits else metric

    # -- transmit side -----------------------------------------------------------
    def _tx_args(self, crc_mask, signal: bool = True):
        """(QpdTxArgs, the mask array it points to) of one transmit call."""
        tx = _lib.QpdTxArgs()
        mask = None
        if crc_mask is not None:
            mask = np.ascontiguousarray(np.asarray(crc_mask).reshape(-1).astype(np.uint8))
            tx.crc_mask, tx.crc_mask_bits = _ptr(mask), mask.size
        tx.no_signal = 0 if signal else 1
        return tx, mask

    def encode_batch(self, msg, crc_mask=None, return_info: bool = False):
        """Encode B messages for this decoder's code: the drivers' ``PolarEnc.encode`` (and, for
        the CRC-aided decoders, ``CRCEnc.encode`` in front of it), batched (qpd_encode /
        qpd_encode_host).  ``msg``: 0/1 entries, [B, A] for the CRC-aided decoders (the first K - A
        bits of the message's CRC are appended), else [B, K].  -> codewords uint8 [B, N], or
        ``(info [B, K], codewords)`` with ``return_info``.  ``crc_mask`` (0/1 entries, at most
        crc_n): XORed onto the tail of the CRC before it is cut to K - A bits, the mirror of
        ``decode_batch(..., return_status=True, crc_mask=...)``: a word encoded under a mask
        passes the CRC only under that mask.  numpy in -> numpy out, on the host; a torch CUDA
        uint8 tensor is read where it lies, on the current stream -> torch CUDA tensors (other
        dtypes are converted to uint8 first).  An entry other than 0 / 1 counts as its low bit
        and raises ValueError (numpy) or is reported by qpd_check_input_error (device)."""
        torch = _torch()
        lib = _lib.load()
        tx, _mask = self._tx_args(crc_mask)
        if torch is not None and isinstance(msg, torch.Tensor) and msg.is_cuda:
            m = msg.reshape(-1, self.A)
            m = (m if m.dtype == torch.uint8 else m.to(torch.uint8)).contiguous()
            B = m.shape[0]
            cw = torch.empty((B, self.N), dtype=torch.uint8, device=m.device)
            info = torch.empty((B, self.K), dtype=torch.uint8, device=m.device) if return_info else None
            stream = torch.cuda.current_stream(m.device).cuda_stream
            _lib.check(lib.qpd_encode(self._h, ctypes.c_void_p(m.data_ptr()), B, ctypes.byref(tx),
                                      None if info is None else ctypes.c_void_p(info.data_ptr()),
                                      ctypes.c_void_p(cw.data_ptr()), ctypes.c_void_p(stream)))
            return (info, cw) if return_info else cw
        if torch is not None and isinstance(msg, torch.Tensor):
            msg = msg.numpy()
        m = np.ascontiguousarray(np.asarray(msg).astype(np.uint8, copy=False).reshape(-1, self.A))
        B = m.shape[0]
        cw = np.empty((B, self.N), dtype=np.uint8)
        info = np.empty((B, self.K), dtype=np.uint8) if return_info else None
        _lib.check(lib.qpd_encode_host(self._h, _ptr(m), B, ctypes.byref(tx), _ptr(info), _ptr(cw)))
        return (info, cw) if return_info else cw

    def transmit_batch(self, msg, sigma: float, seed: int, frame0: int = 0, crc_mask=None, quantizer=None,
                       out: str = "llr", rec=None, signal: bool = True):
        """The received frames of B messages (qpd_tx_frames): ``encode_batch(msg, crc_mask)``,
        BPSK, AWGN of standard deviation ``sigma``, LLR = 2y / sigma^2 -- the frames
        ``montecarlo.GpuFrames`` / ``GpuLlrFrames`` make, for messages the caller chooses.  Row b
        is global frame ``frame0 + b`` of ``seed``: its noise is the generator's for that frame
        id, whatever the batch.  ``out``: "llr" (float64 [B, N]; with ``rec``, one value per
        symbol, the LLRs re-quantised to rec[symbol]), "symbols" (int32) or "symbols_u8"
        (uint8, q <= 256) -- the symbols of ``quantizer``, a :class:`ChannelQuantizer`, which
        "llr" needs only with ``rec``.  ``signal=False``: noise only (y = sigma * noise), an
        empty candidate of a blind detection; ``msg`` then only gives the number of frames (an
        int will do).  Always on the device: a torch CUDA tensor is read where it lies, on the
        current stream -> a torch CUDA tensor; numpy in -> numpy out, through the device.
        Decoding is a second call: ``decode_batch(transmit_batch(...))``."""
        torch = _torch()
        if torch is None:
            raise RuntimeError("transmit_batch runs on the device: it needs torch")
        kinds = {"llr": (_lib.QPD_TX_LLR_F64, torch.float64), "symbols": (_lib.QPD_TX_SYM_I32, torch.int32),
                 "symbols_u8": (_lib.QPD_TX_SYM_U8, torch.uint8)}
        if out not in kinds:
            raise ValueError(f"out must be one of {sorted(kinds)}, got {out!r}")
        ty, dtype = kinds[out]
        if quantizer is not None and not isinstance(quantizer, ChannelQuantizer):
            raise TypeError(f"transmit_batch takes a ChannelQuantizer, got {type(quantizer).__name__}")
        if quantizer is None and (out != "llr" or rec is not None):
            raise ValueError("symbols and rec need a quantizer")
        if rec is not None and out != "llr":
            raise ValueError("rec applies to out='llr' only")
        ch = _lib.QpdMcChannel()
        ch.sigma = float(sigma)
        if quantizer is not None:
            ch.q, ch.n_edges = quantizer.q, quantizer.edges.size
            ch.edges, ch.lut = quantizer.edges.ctypes.data, quantizer.lut.ctypes.data
        recp = None
        if rec is not None:
            recp = np.ascontiguousarray(rec, dtype=np.float64)
            if recp.size < quantizer.q:
                raise ValueError(f"rec must have q={quantizer.q} entries, got {recp.size}")
        tx, _mask = self._tx_args(crc_mask, signal)
        on_device = isinstance(msg, torch.Tensor) and msg.is_cuda
        device = msg.device if on_device else torch.device("cuda", max(self.device, 0))
        if isinstance(msg, (int, np.integer)):
            if signal:
                raise ValueError("a frame count instead of messages needs signal=False")
            B, m = int(msg), None
        else:
            if not isinstance(msg, torch.Tensor):
                msg = torch.from_numpy(np.ascontiguousarray(np.asarray(msg).astype(np.uint8, copy=False)))
            m = msg.reshape(-1, self.A)
            m = (m if m.dtype == torch.uint8 else m.to(torch.uint8)).to(device).contiguous()
            B = m.shape[0]
        frames = torch.empty((B, self.N), dtype=dtype, device=device)
        stream = torch.cuda.current_stream(device).cuda_stream
        _lib.check(_lib.load().qpd_tx_frames(self._h, ctypes.byref(ch), _ptr(recp), ctypes.c_uint64(int(seed)), int(frame0), B,
                                             None if m is None else ctypes.c_void_p(m.data_ptr()), ctypes.byref(tx), ty,
                                             ctypes.c_void_p(frames.data_ptr()), ctypes.c_void_p(stream)))
        return frames if on_device else frames.cpu().numpy()

    # -- LLR input of the LUT decoders ------------------------------------------
    def _llr_args(self, llr, quantizer, name):
        """(device?, contiguous [B, N] array / tensor, llr_type) of an LLR batch."""
        if self._float_input:
            raise TypeError(f"{type(self).__name__} decodes float64 LLRs as they are: use decode_batch, not {name}")
        if not isinstance(quantizer, ChannelQuantizer):
            raise TypeError(f"{name} takes a ChannelQuantizer, got {type(quantizer).__name__}")
        torch = _torch()
        if torch is not None and isinstance(llr, torch.Tensor) and llr.is_cuda:
            if not llr.dtype.is_floating_point:
                raise TypeError(f"{name} takes floating-point LLRs, got {llr.dtype}")
            want = llr.dtype if llr.dtype in (torch.float64, torch.float32) else torch.float64
            xs = llr.reshape(-1, self.N).to(want).contiguous()
            return True, xs, _lib.QPD_LLR_F32 if want == torch.float32 else _lib.QPD_LLR_F64
        if torch is not None and isinstance(llr, torch.Tensor):
            llr = llr.numpy()
        a = np.asarray(llr)
        if a.dtype.kind != "f":
            raise TypeError(f"{name} takes floating-point LLRs, got {a.dtype}")
        want = a.dtype if a.dtype in (np.float64, np.float32) else np.float64
        a = np.ascontiguousarray(a.astype(want, copy=False).reshape(-1, self.N))
        return False, a, _lib.QPD_LLR_F32 if want == np.float32 else _lib.QPD_LLR_F64

    def decode_llr_batch(self, llr, quantizer: "ChannelQuantizer"):
        """Decode B frames of channel LLRs on a LUT decoder: ``quantizer`` (the drivers'
        channel quantizer, q <= v) runs in front of the decode, in the library.  A torch
        CUDA float64 / float32 tensor [B, N] is read where it is (qpd_decode_llr on the
        current stream, no copy) -> torch CUDA uint8 [B, K]; other float dtypes are
        converted to float64; a numpy array goes to qpd_decode_llr_host -> numpy uint8
        [B, K].  The bits are decode_batch's for ``quantizer(llr)``.  A NaN LLR raises
        ValueError (numpy), or is reported by qpd_check_input_error (device)."""
        dev, xs, ty = self._llr_args(llr, quantizer, "decode_llr_batch")
        lib = _lib.load()
        B = xs.shape[0]
        if dev:
            torch = _torch()
            out = torch.empty((B, self.out_bits), dtype=torch.uint8, device=xs.device)
            stream = torch.cuda.current_stream(xs.device).cuda_stream
            _lib.check(lib.qpd_decode_llr(self._h, ctypes.byref(quantizer.ch), ctypes.c_void_p(xs.data_ptr()), ty, B,
                                          ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(stream)))
            return out
        out = np.empty((B, self.out_bits), dtype=np.uint8)
        _lib.check(lib.qpd_decode_llr_host(self._h, ctypes.byref(quantizer.ch), _ptr(xs), ty, B, _ptr(out)))
        return out

    def quantize_llr(self, llr, quantizer: "ChannelQuantizer"):
        """The channel quantizer alone (q <= 256): a torch CUDA tensor [B, N] ->
        torch CUDA uint8 symbols [B, N] on the current stream (qpd_quantize_llr); a
        numpy array -> numpy uint8, through the device."""
        dev, xs, ty = self._llr_args(llr, quantizer, "quantize_llr")
        torch = _torch()
        if not dev:
            if torch is None:
                raise RuntimeError("quantize_llr runs on the device: it needs torch")
            return self.quantize_llr(torch.from_numpy(xs).to(torch.device("cuda", max(self.device, 0))),
                                     quantizer).cpu().numpy()
        out = torch.empty(xs.shape, dtype=torch.uint8, device=xs.device)
        stream = torch.cuda.current_stream(xs.device).cuda_stream
        _lib.check(_lib.load().qpd_quantize_llr(self._h, ctypes.byref(quantizer.ch), ctypes.c_void_p(xs.data_ptr()), ty,
                                                xs.shape[0], ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(stream)))
        return out

    def set_host_engine(self, mode: str = "auto") -> None:
        """Where host-buffer calls (``decode``, numpy ``decode_batch``) run:
        "auto" (the host engine for the few frames a per-frame call brings, the
        GPU for batches; ``info()["host_max_frames"]``), "gpu" or "cpu"."""
        m = {"auto": _lib.QPD_HOST_AUTO, "gpu": _lib.QPD_HOST_GPU, "cpu": _lib.QPD_HOST_CPU}[mode]
        _lib.check(_lib.load().qpd_set_host_engine(self._h, m))

    def _decode_one(self, x) -> np.ndarray:
        # the per-frame call (mainQuantizedDecoder_LLRDomain.py:178): one frame
        # straight to the host-buffer entry point, no batch reshaping; the
        # values are force-cast as pybind11's array_t<int> / <double> does
        a = np.asarray(x).reshape(-1)
        if a.size < self.N:
            raise ValueError(f"decode expects N={self.N} values, got {a.size}")
        with self._one_lock:  # the GIL is released during the call: keep the buffers per call
            np.copyto(self._one_in, a[: self.N], casting="unsafe")
            _lib.check(self._one_fn(self._h, self._one_args[0], 1, self._one_args[1]))
            return self._one_out.copy()


class _LUTDecoder(_DecoderBase):
    def decode(self, channel_quantized_symbols):
        return self._decode_one(channel_quantized_symbols)


class SCLUTDecoder(_LUTDecoder):
    """SC-LUT (SCLUTDecoder.cpp:21-124)."""

    _kind = _lib.QPD_SC_LUT

    def __init__(self, N, K, frozen_bits, message_bits, LUT_f, LUT_g, virtual_channel_llr, **kw):
        super().__init__(N, K, 1, frozen_bits, message_bits, None, pack_luts(int(N), LUT_f, LUT_g, virtual_channel_llr),
                         **kw)


class SCLLUTDecoder(_LUTDecoder):
    """SCL-LUT (SCLLUTDecoder.cpp:47-253)."""

    _kind = _lib.QPD_SCL_LUT

    def __init__(self, N, K, L, frozen_bits, message_bits, LUT_f, LUT_g, virtual_channel_llr, **kw):
        super().__init__(N, K, L, frozen_bits, message_bits, None, pack_luts(int(N), LUT_f, LUT_g, virtual_channel_llr),
                         **kw)


class FastSCLUTDecoder(_DecoderBase):
    """FastSC-LUT (FastSCLUT.cpp:27-206); note the reference's kwargs LUT_Fs/LUT_Gs
    and decode(llr) (py_FastSCLUTDecoder.cpp:12-15)."""

    _kind = _lib.QPD_FASTSC_LUT

    def __init__(self, N, K, frozen_bits, message_bits, node_type, LUT_Fs, LUT_Gs, virtual_channel_llr, **kw):
        super().__init__(N, K, 1, frozen_bits, message_bits, node_type,
                         pack_luts(int(N), LUT_Fs, LUT_Gs, virtual_channel_llr), **kw)

    def decode(self, llr):
        return self._decode_one(llr)


class FastSCLLUTDecoder(_LUTDecoder):
    """FastSCL-LUT (FastSCLLUTDecoder.cpp:57-408)."""

    _kind = _lib.QPD_FASTSCL_LUT

    def __init__(self, N, K, L, frozen_bits, message_bits, node_type, LUT_f, LUT_g, virtual_channel_llr, **kw):
        super().__init__(N, K, L, frozen_bits, message_bits, node_type,
                         pack_luts(int(N), LUT_f, LUT_g, virtual_channel_llr), **kw)


class CASCLLUTDecoder(_LUTDecoder):
    """CRC-aided SCL-LUT (CASCLLUTDecoder.cpp:64-303; ctor py_CASCLLUTDecoder.cpp:10-17).
    ``decode`` returns the A message bits.  Like the reference, ``crc_n``/``crc_p``
    are accepted and stored but the check is always CRC-24 (CRC24_LOC)."""

    _kind = _lib.QPD_CASCL_LUT

    def __init__(self, N, K, A, L, frozen_bits, message_bits, crc_n, crc_p, LUT_f, LUT_g, virtual_channel_llr, **kw):
        self.crc_n, self.crc_p = crc_n, crc_p
        super().__init__(N, K, L, frozen_bits, message_bits, None, pack_luts(int(N), LUT_f, LUT_g, virtual_channel_llr),
                         A=A, **kw)


class CAFastSCLLUTDecoder(_LUTDecoder):
    """CRC-aided FastSCL-LUT (CAFastSCLLUTDecoder.cpp:58-454; ctor
    py_CAFastSCLLUTDecoder.cpp:10-16).  ``decode`` returns the A message bits."""

    _kind = _lib.QPD_CAFASTSCL_LUT

    def __init__(self, N, K, A, L, frozen_bits, message_bits, node_type, LUT_f, LUT_g, virtual_channel_llr, **kw):
        super().__init__(N, K, L, frozen_bits, message_bits, node_type,
                         pack_luts(int(N), LUT_f, LUT_g, virtual_channel_llr), A=A, **kw)


class SCDecoder(_DecoderBase):
    """Float SC, min-sum on float64 LLRs (SCDecoder.cpp:14-89)."""

    _kind = _lib.QPD_SC_FLOAT

    def __init__(self, N, K, frozen_bits, message_bits, **kw):
        super().__init__(N, K, 1, frozen_bits, message_bits, None, None, **kw)

    def decode(self, llr):
        return self._decode_one(llr)


class _FloatDecoder(_DecoderBase):
    def decode(self, llr):
        return self._decode_one(llr)


class SCLDecoder(_FloatDecoder):
    """Float SCL, min-sum list decoding on float64 LLRs (SCLDecoder.cpp:38-176)."""

    _kind = _lib.QPD_SCL_FLOAT

    def __init__(self, N, K, L, frozen_bits, message_bits, **kw):
        super().__init__(N, K, L, frozen_bits, message_bits, None, None, **kw)


class CASCLDecoder(_FloatDecoder):
    """CRC-aided float SCL (CASCLDecoder.cpp:74-249; ctor py_CASCLDecoder.cpp:10-12).
    Unlike the CA-LUT classes it checks the CRC it is given: ``crc_n`` bits with
    divisor coefficients ``crc_p`` (a list of indices, CASCLDecoder.cpp:49-53).
    ``decode`` returns the A message bits."""

    _kind = _lib.QPD_CASCL_FLOAT

    def __init__(self, N, K, A, L, frozen_bits, message_bits, crc_n, crc_p, **kw):
        self.crc_n, self.crc_p = int(crc_n), list(crc_p)
        super().__init__(N, K, L, frozen_bits, message_bits, None, None, A=A, crc_n=int(crc_n), crc_loc=crc_p, **kw)


class FastSCDecoder(_FloatDecoder):
    """Float Fast-SC with R0/R1/REP/SPC nodes (FastSCDecoder.cpp:21-174)."""

    _kind = _lib.QPD_FASTSC_FLOAT

    def __init__(self, N, K, frozen_bits, message_bits, node_type, **kw):
        super().__init__(N, K, 1, frozen_bits, message_bits, node_type, None, **kw)


class FastSCLDecoder(_FloatDecoder):
    """Float Fast-SCL with R0/R1/REP nodes, no SPC (FastSCLDecoder.cpp:49-423)."""

    _kind = _lib.QPD_FASTSCL_FLOAT

    def __init__(self, N, K, L, frozen_bits, message_bits, node_type, **kw):
        super().__init__(N, K, L, frozen_bits, message_bits, node_type, None, **kw)


class SCUniformQuantizedDecoder(_FloatDecoder):
    """SC with uniform re-quantization after every f/g (SCUniformQuantizedDecoder.cpp:20-99)."""

    _kind = _lib.QPD_SC_UNIFORM

    def __init__(self, N, K, frozen_bits, message_bits, decoder_r_f, decoder_r_g, v, **kw):
        super().__init__(N, K, 1, frozen_bits, message_bits, None, None,
                         quant=pack_uniform(int(N), decoder_r_f, decoder_r_g, int(v)), **kw)


class SCLUniformQuantizedDecoder(_FloatDecoder):
    """SCL with uniform re-quantization (SCLUniformQuantizedDecoder.cpp:43-184)."""

    _kind = _lib.QPD_SCL_UNIFORM

    def __init__(self, N, K, L, frozen_bits, message_bits, decoder_r_f, decoder_r_g, v, **kw):
        super().__init__(N, K, L, frozen_bits, message_bits, None, None,
                         quant=pack_uniform(int(N), decoder_r_f, decoder_r_g, int(v)), **kw)


class SCLloydQuantizedDecoder(_FloatDecoder):
    """SC with Lloyd re-quantization after every f/g (SCLloydQuantizedDecoder.cpp:22-101)."""

    _kind = _lib.QPD_SC_LLOYD

    def __init__(self, N, K, frozen_bits, message_bits, boundaries_f, boundaries_g, reconstruction_f,
                 reconstruction_g, v, **kw):
        super().__init__(N, K, 1, frozen_bits, message_bits, None, None,
                         quant=pack_lloyd(int(N), boundaries_f, boundaries_g, reconstruction_f, reconstruction_g,
                                          int(v)), **kw)


class SCLLloydQuantizedDecoder(_FloatDecoder):
    """SCL with Lloyd re-quantization (SCLLloydQuantizedDecoder.cpp:46-187)."""

    _kind = _lib.QPD_SCL_LLOYD

    def __init__(self, N, K, L, frozen_bits, message_bits, boundaries_f, boundaries_g, reconstruction_f,
                 reconstruction_g, v, **kw):
        super().__init__(N, K, L, frozen_bits, message_bits, None, None,
                         quant=pack_lloyd(int(N), boundaries_f, boundaries_g, reconstruction_f, reconstruction_g,
                                          int(v)), **kw)


FLOAT_CLASSES = {"SC": SCDecoder, "SCL": SCLDecoder, "CA-SCL": CASCLDecoder, "FastSC": FastSCDecoder,
                 "FastSCL": FastSCLDecoder, "SC-Uniform": SCUniformQuantizedDecoder,
                 "SCL-Uniform": SCLUniformQuantizedDecoder, "SC-Lloyd": SCLloydQuantizedDecoder,
                 "SCL-Lloyd": SCLLloydQuantizedDecoder}


def from_quant(kind: str, N: int, K: int, frozen_bits, L: int = 1, node_type=None, quant=None, **kw):
    """Build a float-domain decoder (kind as oracle.FLOAT_KIND) from packed re-quantizers."""
    cls = FLOAT_CLASSES[kind]
    obj = cls.__new__(cls)
    lst = kind in ("SCL", "CA-SCL", "FastSCL", "SCL-Uniform", "SCL-Lloyd")
    _DecoderBase.__init__(obj, N, K, L if lst else 1, frozen_bits, 1 - np.asarray(frozen_bits), node_type, None,
                          quant=quant, **kw)
    return obj


def from_packed(kind: str, packed: PackedLUT, K: int, frozen_bits, L: int = 1, node_type=None, **kw):
    """Build a decoder directly from packed tables (skips the nested-list path)."""
    cls = {"SC-LUT": SCLUTDecoder, "SCL-LUT": SCLLUTDecoder, "FastSC-LUT": FastSCLUTDecoder,
           "FastSCL-LUT": FastSCLLUTDecoder, "CA-SCL-LUT": CASCLLUTDecoder,
           "CA-FastSCL-LUT": CAFastSCLLUTDecoder}[kind]
    obj = cls.__new__(cls)
    lst = kind in ("SCL-LUT", "FastSCL-LUT", "CA-SCL-LUT", "CA-FastSCL-LUT")
    _DecoderBase.__init__(obj, packed.N, K, L if lst else 1, frozen_bits, 1 - np.asarray(frozen_bits), node_type, packed,
                          **kw)
    return obj
