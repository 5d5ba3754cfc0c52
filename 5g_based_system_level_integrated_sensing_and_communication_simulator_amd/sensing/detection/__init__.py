from .cfar2D import cfar2D, CFARDetector2D  # noqa: F401
from .cfarDetect import cfarDetect, cfarThresholdFactor  # noqa: F401
from .cfarMonteCarlo import cfarMonteCarlo  # noqa: F401
from .getPd import getPd  # noqa: F401
