# Same shape as the reference (PolarBD/PolarBD/__init__.py).
from . import CASCLWithRNTI, DMetricCalculator  # noqa: F401
