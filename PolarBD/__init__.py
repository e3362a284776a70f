"""Drop-in replacement for the reference package ``PolarBD``
(PolarEncoder/PolarBD): the same module path and class name for its float CA-SCL
decoder with RNTI, decoding through libqpd.so.  ``DMetricCalculator`` is not
provided."""
from . import PolarBD  # noqa: F401
from quantized_decoder_polar_codes_amd import __version__  # noqa: F401
