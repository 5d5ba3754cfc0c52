"""tools (the reference's +tools package): the helpers its sensing functions call."""
from .find2DPeaks import find2DPeaks  # noqa: F401
