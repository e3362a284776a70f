# Same shape as the reference (PolarBD/PolarBD/__init__.py), without DMetricCalculator.
from . import CASCLWithRNTI  # noqa: F401
