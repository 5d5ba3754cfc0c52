"""Mirror of the reference's ``+communication`` package (hot-path seams only)."""
from . import channelModels, pathlossModels, phyLayer  # noqa: F401
