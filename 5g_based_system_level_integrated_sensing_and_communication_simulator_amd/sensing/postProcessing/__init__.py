from .getRMSE import getRMSE  # noqa: F401
