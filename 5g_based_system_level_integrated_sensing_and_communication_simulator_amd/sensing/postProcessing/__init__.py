from .getRMSE import getRMSE  # noqa: F401
from .getPositionRMSE import getPositionRMSE  # noqa: F401
from .getTrackRMSE import getTrackRMSE  # noqa: F401
