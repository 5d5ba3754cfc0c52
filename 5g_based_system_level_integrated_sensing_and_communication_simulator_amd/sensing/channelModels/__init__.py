from .basicRadarChannel import basicRadarChannel  # noqa: F401
from .multiStaticChannel import multiStaticChannel, multiStaticPaths  # noqa: F401
from .referencePaths import referencePaths  # noqa: F401
