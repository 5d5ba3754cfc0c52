"""tools.find2DPeaks(PdB, L): called by the UPA branches of music.m:69, digitalBF.m:51 and mvdrBF.m:51, never defined by the reference.
The project's definition (include/isac.h, isac_find2d_peaks): interior cells strictly above all 8 neighbours, sorted by
value (descending, ties by column-major index), the first min(L, #) of them."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib as L


def find2DPeaks(PdB, numPeaks, *, ctx=None):
    """[ele, azi] = tools.find2DPeaks(PdB, L): 1-based row (elevation) and column (azimuth) indices of the peaks of the matrix PdB.
    numPeaks <= 0 raises IsacError(NO_DETECTION), as findpeaks' 'NPeaks' does on the ULA path."""
    ctx = ctx or L.default_context()
    p = np.asfortranarray(np.asarray(PdB, dtype=np.float64))
    if p.ndim != 2:
        raise ValueError("PdB must be a matrix")
    rows, cols = p.shape
    n = max(int(numPeaks), 0)
    ele = np.zeros(max(n, 1), dtype=np.int32)
    azi = np.zeros(max(n, 1), dtype=np.int32)
    found = C.c_int32(0)
    ctx.check(ctx.lib.isac_find2d_peaks(ctx.handle, p.ctypes.data_as(C.c_void_p), rows, cols, int(numPeaks),
                                        ele.ctypes.data_as(C.c_void_p), azi.ctypes.data_as(C.c_void_p), C.byref(found)))
    k = found.value
    return ele[:k].astype(np.int64), azi[:k].astype(np.int64)
