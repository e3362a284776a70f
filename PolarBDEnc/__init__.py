"""Drop-in replacement for the package every reference driver imports and the
reference does not ship, ``PolarBDEnc``: the same module paths and class names for
the two classes the drivers use,

    from PolarBDEnc.Encoder.PolarEnc import PolarEnc    # PolarEnc(N, K, frozenbits, msgbits).encode(msg)
    from PolarBDEnc.Encoder.CRCEnc import CRCEnc        # CRCEnc(crc_n, crc_p).encode(msg)

(mainQuantizedDecoder_LLRDomain.py:10-11, :72-73, :153-158), on libqpd.so's encoder
(qpd_encode_host / qpd_encode, include/qpd.h)."""
from . import Encoder  # noqa: F401
from quantized_decoder_polar_codes_amd import __version__  # noqa: F401
