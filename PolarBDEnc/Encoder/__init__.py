# The submodules are imported, each holding its class of the same name (as PolarDecoder/Decoder).
from . import CRCEnc, PolarEnc  # noqa: F401
