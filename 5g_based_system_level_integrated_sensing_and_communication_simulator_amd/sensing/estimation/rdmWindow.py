"""sensing.estimation.rdmWindow: the complex range-Doppler window of the last fft2D call (project-defined; include/isac_beams.h, isac_fft2d_get_rdm_window)."""
from __future__ import annotations

import ctypes as C

import numpy as np


def rdmWindow(ctx):
    """``(Y, first_row, first_col)``: Y [nr x nc x A] = rdm(r, c, a) on the cells of the power window of the last completed fft2D on ``ctx`` (the CUT zone plus its halo
    of guard + training cells); Y[0, 0, :] is rdm cell (first_row, first_col), 1-based.  |Y|^2 is the power window; the snapshots of sensing.estimation.targetList are
    Y at the listed cells, bit for bit.  Raises IsacError(INVALID_ARG) when no completed fft2D is left on the context (or a later call has rewritten its range rows)."""
    lib = ctx.lib
    dims = (C.c_int32 * 3)()
    fr, fc = C.c_int32(0), C.c_int32(0)
    ctx.check(lib.isac_fft2d_get_rdm_window(ctx.handle, None, 0, dims, C.byref(fr), C.byref(fc)))
    y = np.zeros(tuple(dims), dtype=np.complex128, order="F")
    ctx.check(lib.isac_fft2d_get_rdm_window(ctx.handle, y.ctypes.data_as(C.c_void_p), y.size, dims, C.byref(fr), C.byref(fc)))
    return y, int(fr.value), int(fc.value)
