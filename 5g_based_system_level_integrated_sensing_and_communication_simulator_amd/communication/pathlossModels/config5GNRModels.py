"""communication.pathlossModels.config5GNRModels (+communication/+pathlossModels/config5GNRModels.m): TR 38.901 7.4.1 path loss through the library's
``isac_path_loss_38901`` (host-side scalar, no GPU)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _lib as L

# the nine nrPathLossConfig scenarios config5GNRModels.m:8-25 lists -> isac_path_loss_scenario
SCENARIOS = {"UMa": 0, "UMi": 1, "RMa": 2, "InH": 3, "InF-SL": 4, "InF-DL": 5, "InF-SH": 6, "InF-DH": 7, "InF-HH": 8}


def _pos(p):
    a = np.ascontiguousarray(np.asarray(p, dtype=np.float64).reshape(-1))
    if a.size != 3:
        raise ValueError("a position is [x y z]")
    return a


def config5GNRModels(pathLossConfig, carrierFreq, losCondition, bsPosition, uePosition, *, BuildingHeight=5.0, StreetWidth=20.0,
                     EnvironmentHeight=1.0, OptionalModel=False):
    """pathLoss [dB] = nrPathLoss(nrPathLossConfig('Scenario', pathLossConfig), carrierFreq, losCondition, bsPosition', uePosition'); 0 for equal positions
    (config5GNRModels.m:32-33).  ``pathLossConfig``: the scenario string.  The keyword arguments are nrPathLossConfig's other properties at their defaults (the reference
    never sets them).  The third coordinate of ``bsPosition`` is h_BS and of ``uePosition`` h_UT, in the order PASSED: uePhy.m:744 passes the UE's own position first
    (the downlink evaluates the model with the heights swapped), gNBPhy.m:853 the gNB's -- a caller that wants the reference's numbers passes them the same way."""
    if pathLossConfig not in SCENARIOS:
        raise ValueError(f"pathLossConfig must be one of {sorted(SCENARIOS)} (config5GNRModels.m:8-25)")
    cfg = L.PathLossConfig(float(BuildingHeight), float(StreetWidth), float(EnvironmentHeight), 1 if OptionalModel else 0, 0)
    bs, ue = _pos(bsPosition), _pos(uePosition)
    out = C.c_double(0.0)
    st = L.load().isac_path_loss_38901(SCENARIOS[pathLossConfig], float(carrierFreq), 1 if losCondition else 0,
                                       bs.ctypes.data_as(C.c_void_p), ue.ctypes.data_as(C.c_void_p), C.byref(cfg), C.byref(out))
    if st != 0:
        raise L.IsacError(st, "isac_path_loss_38901: carrier frequency must be positive")
    return out.value
