"""``CRCEnc`` of the drivers (mainQuantizedDecoder_LLRDomain.py:73, :156):
``CRCEnc(crc_n, crc_p).encode(msg) -> ndarray[A + crc_n]``, the message followed by its
check code (CRC::encoding, utils.cpp:77-92); ``crc_p`` is the list of the divisor's
coefficient indices the drivers pass (crc_p[i] = 1 for i in the list, index 0 the leading
one -- the ``crc_p`` of CASCLDecoder).  Host code: the shift register is linear in the
message bits, so the check code is the XOR of one precomputed row per set bit, the table the
library's encoder uses (csrc/qpd_tx.hpp), built per message length at the first call.

``encode_batch(msg[B, A]) -> uint8 [B, A + crc_n]`` is the addition.  Frames for a CRC-aided
decoder come from that decoder in one step: ``encode_batch`` / ``transmit_batch`` of the
CASCLLUTDecoder, CAFastSCLLUTDecoder and CASCLDecoder classes append the CRC themselves,
optionally scrambled with an RNTI.
"""
import numpy as np


class CRCEnc:
    def __init__(self, crc_n, crc_p):
        self.crc_n = int(crc_n)
        self.crc_p = [int(j) for j in crc_p]
        if self.crc_n < 1 or any(j < 0 or j > self.crc_n for j in self.crc_p):
            raise ValueError("crc_p entries must be in [0, crc_n]")
        self._taps = np.zeros(self.crc_n, dtype=np.uint8)  # coefficient j >= 1 -> check bit j - 1 of a lone last bit
        for j in self.crc_p:
            if j >= 1:
                self._taps[j - 1] = 1
        self._tabs = {}

    def _table(self, A):
        """[A, crc_n]: the check code of message bit j alone (row A-1 = the taps; row j = one zero
        step of row j+1: shift towards the leading bit, XOR the taps if it falls out)."""
        tab = self._tabs.get(A)
        if tab is None:
            tab = np.zeros((A, self.crc_n), dtype=np.uint8)
            if A:
                tab[A - 1] = self._taps
            for j in range(A - 2, -1, -1):
                r = tab[j + 1]
                tab[j, :-1] = r[1:]
                if r[0]:
                    tab[j] ^= self._taps
            self._tabs[A] = tab
        return tab

    def encode_batch(self, msg):
        m = np.asarray(msg)
        m = (m.reshape(-1, m.shape[-1]) & 1).astype(np.uint8)
        crc = (m.astype(np.int64) @ self._table(m.shape[1]).astype(np.int64)) & 1
        return np.concatenate([m, crc.astype(np.uint8)], axis=1)

    def encode(self, msg):
        return self.encode_batch(np.asarray(msg).reshape(1, -1))[0]
