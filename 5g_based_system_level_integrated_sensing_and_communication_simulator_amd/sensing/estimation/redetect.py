"""sensing.estimation.redetect: the last fft2D call detected again with another CFAR method (include/isac_cfar.h, isac_fft2d_redetect)."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np

from ... import _lib as L
from ..detection.cfarDetect import method_block
from ._cpi_post import cpi_dims
from .doaEstimation.music import music


def redetect(ctx, Method="CA", Rank=1, ThresholdFactor="Auto", CustomThresholdFactor=None, return_debug=False, radarEstParams=None):
    """estResults of the last completed fft2D on ``ctx`` with its CFAR stage run again as ``Method`` ('CA', 'GOCA', 'SOCA', 'OS'; ``Rank`` for 'OS') and
    ``ThresholdFactor`` 'Auto' or 'Custom': the power window that call left on the device is detected again, fft2D.m:63-99 give ``rngEst, velEst`` and numDets, and
    ``aziEst, eleEst`` come from the call's covariance through sensing.estimation.doaEstimation.music with the new numDets (fft2D.m:110-111) and the scan grid of
    the radarEstParams that fft2D call was given (``radarEstParams`` overrides them; needed after sensing.submitN, which keeps none).  ``return_debug`` adds a namespace with the per-antenna ``detections`` ([2 x D] 1-based, CUT order), ``det_pow``,
    ``numDets`` and ``totalDetections``.  Raises IsacError(INVALID_ARG) when no completed fft2D is left on the context, IsacError(NO_DETECTION) from music when nothing is
    detected."""
    lib = ctx.lib
    radarEstParams = radarEstParams if radarEstParams is not None else getattr(ctx, "fft2d_radar_params", None)
    if radarEstParams is None:
        raise ValueError("redetect: this context has run no fft2D through sensing.estimation.fft2D; pass radarEstParams")
    m = method_block(Method, Rank, ThresholdFactor, CustomThresholdFactor)
    A = cpi_dims(ctx)[2]
    res = L.EstResult()
    off = np.zeros(A + 1, dtype=np.int32)
    n_total = C.c_int32(0)
    ctx.check(lib.isac_fft2d_redetect(ctx.handle, C.byref(m), C.byref(res), None, None, 1 << 30, off.ctypes.data_as(C.c_void_p), C.byref(n_total)))
    ra = np.zeros((A, A), dtype=np.complex128, order="F")
    ctx.check(lib.isac_fft2d_get_covariance(ctx.handle, ra.ctypes.data_as(C.c_void_p), A))
    dbg = None
    if return_debug:
        n = int(n_total.value)
        idx = np.zeros((2, max(n, 1)), dtype=np.int32, order="F")
        pw = np.zeros(max(n, 1), dtype=np.float64)
        ctx.check(lib.isac_fft2d_redetect(ctx.handle, C.byref(m), C.byref(res), idx.ctypes.data_as(C.c_void_p), pw.ctypes.data_as(C.c_void_p), max(n, 1),
                                          off.ctypes.data_as(C.c_void_p), C.byref(n_total)))
        dbg = SimpleNamespace(detections=[idx[:, off[a]:off[a + 1]].astype(np.int64) for a in range(A)], det_pow=[pw[off[a]:off[a + 1]] for a in range(A)],
                              numDets=int(res.num_dets), totalDetections=int(res.total_detections), Ra=ra)
    _, azi, ele = music(int(res.num_dets), radarEstParams, ra, ctx=ctx)
    est = SimpleNamespace(rngEst=np.array(res.rng_est[: res.n_rng]), velEst=np.array(res.vel_est[: res.n_vel]), aziEst=azi, eleEst=ele)
    return (est, dbg) if return_debug else est
