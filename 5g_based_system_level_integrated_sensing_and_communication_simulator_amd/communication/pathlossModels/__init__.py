"""Mirror of the reference's ``+communication/+pathlossModels``: the two functions that give ``pathLoss`` in applyChannelModel (uePhy.m:742-747, gNBPhy.m:851-856)."""
from .config5GNRModels import config5GNRModels, SCENARIOS  # noqa: F401
from .configFreeSpaceModel import configFreeSpaceModel  # noqa: F401
