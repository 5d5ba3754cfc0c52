"""The detectors phased.CFARDetector2D offers besides cell averaging (cfar2D.m:28-29 names them): Method 'CA' / 'GOCA' / 'SOCA' / 'OS', ThresholdFactor 'Auto' / 'Custom'
(include/isac_cfar.h: isac_cfar2d, isac_cfar_threshold_factor; project-defined where the toolbox is silent)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _lib as L


def method_block(Method="CA", Rank=1, ThresholdFactor="Auto", CustomThresholdFactor=None) -> L.CfarMethod:
    """The detector's Method / Rank / ThresholdFactor / CustomThresholdFactor properties -> isac_cfar_method."""
    if Method not in L.CFAR_METHODS:
        raise ValueError(f"Method must be one of {list(L.CFAR_METHODS)}")
    if ThresholdFactor == "Auto":
        factor = 0.0
    elif ThresholdFactor == "Custom":
        if CustomThresholdFactor is None:
            raise ValueError("ThresholdFactor 'Custom' needs CustomThresholdFactor")
        factor = float(CustomThresholdFactor)
        if factor == 0.0:
            raise ValueError("CustomThresholdFactor must be positive")
    else:
        raise ValueError("ThresholdFactor must be 'Auto' or 'Custom' ('Input port' is not offered)")
    return L.CfarMethod(L.CFAR_METHODS[Method], int(Rank), factor)


def cfarThresholdFactor(Method, nTrain, Pfa, Rank=1) -> float:
    """The 'Auto' threshold factor of ``Method`` for ``nTrain`` training cells (host only: needs no GPU)."""
    if Method not in L.CFAR_METHODS:
        raise ValueError(f"Method must be one of {list(L.CFAR_METHODS)}")
    alpha = C.c_double(0.0)
    st = L.load().isac_cfar_threshold_factor(L.CFAR_METHODS[Method], int(nTrain), int(Rank), float(Pfa), C.byref(alpha))
    if st != 0:
        raise L.IsacError(st, f"isac_cfar_threshold_factor({Method}, nTrain={nTrain}, Rank={Rank}, Pfa={Pfa})")
    return alpha.value


def cfarDetect(P, CUTIdx, cfarConfig, Method="CA", Rank=1, ThresholdFactor="Auto", CustomThresholdFactor=None, ctx=None):
    """``detections = cfarDetector2D(P, CUTIdx)`` with the detector of ``cfarConfig`` (sensing.detection.cfar2D) switched to another Method / ThresholdFactor:
    [2 x D] 1-based indices in CUT order.  Guard band, training band and ProbabilityFalseAlarm are the configured detector's."""
    det = cfarConfig.cfarDetector2D
    m = method_block(Method, Rank, ThresholdFactor, CustomThresholdFactor)
    ctx = ctx or L.default_context()
    p = np.asfortranarray(np.asarray(P, dtype=np.float64))
    cut = np.asfortranarray(np.asarray(CUTIdx, dtype=np.int32))       # [2 x nCUT] column-major == interleaved (row, col)
    n_cut = cut.shape[1] if cut.ndim == 2 else 0
    out = np.zeros((2, max(n_cut, 1)), dtype=np.int32, order="F")
    n_det = C.c_int32(0)
    g = (C.c_int32 * 2)(*det.GuardBandSize)
    t = (C.c_int32 * 2)(*det.TrainingBandSize)
    ctx.check(ctx.lib.isac_cfar2d(ctx.handle, p.ctypes.data_as(C.c_void_p), p.shape[0], p.shape[1], cut.ctypes.data_as(C.c_void_p), n_cut, g, t,
                                  det.ProbabilityFalseAlarm, C.byref(m), out.ctypes.data_as(C.c_void_p), max(n_cut, 1), C.byref(n_det)))
    return out[:, : n_det.value].astype(np.int64)
