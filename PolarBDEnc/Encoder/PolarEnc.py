"""``PolarEnc`` of the drivers (mainQuantizedDecoder_LLRDomain.py:72, :157-159):
``PolarEnc(N, K, frozenbits, msgbits).encode(msg) -> ndarray[N]``, u[msgbits] = msg,
frozen positions 0, x = u F^{(x)n} in natural order.  ``frozenbits`` and ``msgbits`` are
the index lists the drivers' code constructor returns.  It sits on a QPD_SC_FLOAT handle
for that code and qpd_encode_host / qpd_encode (include/qpd.h).

``encode(msg)`` is the drivers' call, one message of K bits, on the host.
``encode_batch(msg[B, K])`` is the addition: numpy in -> numpy uint8 [B, N] on the host; a
torch CUDA tensor in -> a torch CUDA tensor on the current stream
(``SCDecoder.encode_batch``).
"""
import numpy as np

from quantized_decoder_polar_codes_amd import _lib
from quantized_decoder_polar_codes_amd.decoders import SCDecoder as _SC


class PolarEnc:
    def __init__(self, N, K, frozenbits, msgbits, **kw):
        N, K = int(N), int(K)
        pos = np.asarray(msgbits, dtype=np.int64).reshape(-1)
        if pos.size != K or np.unique(pos).size != K or (K and (pos.min() < 0 or pos.max() >= N)):
            raise ValueError(f"msgbits must be K={K} distinct positions in [0, N)")
        frozen = np.ones(N, dtype=np.int32)
        frozen[pos] = 0
        self.N, self.K = N, K
        self.frozenbits, self.msgbits = np.asarray(frozenbits), pos
        # message bit i sits at position msgbits[i]; the library deposits the information bits in
        # ascending position order
        self._order = None if (np.diff(pos) > 0).all() else np.argsort(pos)
        self._dec = _SC(N, K, frozen, 1 - frozen, **kw)
        self._in = np.empty(K, dtype=np.uint8)
        self._out = np.empty(N, dtype=np.uint8)

    def _ordered(self, m):
        return m if self._order is None else m[..., self._order]

    def encode(self, msg):
        a = np.asarray(msg).reshape(-1)
        if a.size < self.K:
            raise ValueError(f"encode expects K={self.K} bits, got {a.size}")
        d = self._dec
        with d._one_lock:
            np.copyto(self._in, self._ordered(a[: self.K]), casting="unsafe")
            _lib.check(_lib.load().qpd_encode_host(d._h, self._in.ctypes.data, 1, None, None, self._out.ctypes.data))
            return self._out.copy()

    def encode_batch(self, msg):
        if self._order is None:
            return self._dec.encode_batch(msg)
        if isinstance(msg, np.ndarray) or not hasattr(msg, "is_cuda"):
            return self._dec.encode_batch(np.asarray(msg).reshape(-1, self.K)[:, self._order])
        import torch

        return self._dec.encode_batch(msg.reshape(-1, self.K)[:, torch.as_tensor(self._order, device=msg.device)])
