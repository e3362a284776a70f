"""``CASCLDecoder`` of the reference's blind-detection package
(PolarBD/_cpp/py_interface/py_CASCLWithRNTI.cpp; CASCLWithRNTI.cpp:74-252): the float
CA-SCL decoder whose ``decode(llr, RNTI)`` XORs the RNTI onto the tail of the
computed CRC before the compare and returns ``(bits, PM, isPass)``.  It sits on
QPD_CASCL_FLOAT and qpd_decode_status_host (include/qpd.h).

Two differences from the reference, neither visible for a usable code:
* PM is the output path's own metric; the reference returns PML[rank of the
  winner], the same number whenever the last position is an information bit.
* The reference starts dead paths at 1e30 here (CASCLDecoder: 1e300, as the
  library).  Every comparison comes out the same, both absorb any realistic
  increment; only the PM of a dead path that wins could differ, which needs
  2^K < L -- refused with ValueError.
"""
import ctypes

import numpy as np

from quantized_decoder_polar_codes_amd import _lib
from quantized_decoder_polar_codes_amd.decoders import CASCLDecoder as _CASCL


class CASCLDecoder(_CASCL):
    def __init__(self, N, K, A, L, frozen_bits, message_bits, crc_n, crc_p, **kw):
        if K < 31 and (1 << int(K)) < int(L):
            raise ValueError(f"2^K < L (K={K}, L={L}): a dead path (initial metric 1e30 in the reference, 1e300 "
                             "here) could win, and its PM would differ")
        super().__init__(N, K, A, L, frozen_bits, message_bits, crc_n, crc_p, **kw)
        self._bd_in = np.empty(self.N, dtype=np.float64)
        self._bd_out = np.empty(self.out_bits, dtype=np.uint8)
        self._bd_pm = np.zeros(1, dtype=np.float64)
        self._bd_ok = np.zeros(1, dtype=np.uint8)

    def decode(self, llr, RNTI):
        a = np.asarray(llr).reshape(-1)
        if a.size < self.N:
            raise ValueError(f"decode expects N={self.N} values, got {a.size}")
        mask = np.ascontiguousarray(np.asarray(RNTI).reshape(-1).astype(np.uint8) & 1)
        sa = _lib.QpdStatusArgs()
        sa.crc_mask, sa.crc_mask_bits = (mask.ctypes.data if mask.size else None), mask.size
        with self._one_lock:
            np.copyto(self._bd_in, a[: self.N], casting="unsafe")
            sa.metric, sa.crc_pass = self._bd_pm.ctypes.data, self._bd_ok.ctypes.data
            _lib.check(_lib.load().qpd_decode_status_host(self._h, self._bd_in.ctypes.data, _lib.QPD_IN_F64, 1,
                                                          self._bd_out.ctypes.data, ctypes.byref(sa)))
            return self._bd_out.copy(), float(self._bd_pm[0]), bool(self._bd_ok[0])
