"""communication.pathlossModels.configFreeSpaceModel (+communication/+pathlossModels/configFreeSpaceModel.m): free-space path loss through ``isac_path_loss_fspl``."""
from __future__ import annotations

import ctypes as C

from ... import _lib as L
from .config5GNRModels import _pos


def configFreeSpaceModel(carrierFreq, bsPosition, uePosition):
    """pathLoss [dB] = fspl(norm(uePosition - bsPosition), c / carrierFreq) = 20 log10(4 pi R / lambda), negative values (R < lambda / 4 pi, R = 0) clamped to 0."""
    bs, ue = _pos(bsPosition), _pos(uePosition)
    out = C.c_double(0.0)
    st = L.load().isac_path_loss_fspl(float(carrierFreq), bs.ctypes.data_as(C.c_void_p), ue.ctypes.data_as(C.c_void_p), C.byref(out))
    if st != 0:
        raise L.IsacError(st, "isac_path_loss_fspl: carrier frequency must be positive")
    return out.value
