from .fft2D import fft2D, fft2D_submit, fft2D_collect  # noqa: F401
from .targetList import targetList  # noqa: F401
from .targetListUPA import targetListUPA  # noqa: F401
from .redetect import redetect  # noqa: F401
from .rdmWindow import rdmWindow  # noqa: F401
from .beamWeights import beamWeights  # noqa: F401
from .beamDetect import beamDetect  # noqa: F401
from .refineTargets import refineTargets  # noqa: F401
from .refineRange import refineRange  # noqa: F401
from .linkMeasurements import linkMeasurements  # noqa: F401
from .localizeTargets import localizeTargets  # noqa: F401
from .trackMeasurements import trackMeasurements  # noqa: F401
from .trackTargets import Tracker, trackTargets  # noqa: F401
from .cleanTargets import cleanTargets  # noqa: F401
from .beamClean import beamClean  # noqa: F401
from .relaxTargets import relaxTargets  # noqa: F401
from .resolveDirections import resolveDirections  # noqa: F401
from . import doaEstimation  # noqa: F401
from .music2D import music2D  # noqa: F401
