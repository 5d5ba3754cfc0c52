"""sensing.estimation.targetList: the per-target list of the last fft2D call (project-defined; include/isac_targets.h, isac_fft2d_get_targets)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _lib as L


def targetList(ctx, snapshots=False):
    """Paired (range, velocity, azimuth) entries of the last completed fft2D on ``ctx``, strongest first.

    fft2D's own rngEst / velEst / aziEst are three unrelated lists; this joins them per detection: the power window is summed over the antennas, CFAR detections are
    thinned to local maxima, and each surviving cell's array snapshot is scanned for its direction (Bartlett, on MUSIC's ULA grid).  Returns a dict of NumPy arrays
    ``rng, vel, azi, power, hits, row, col`` (1-based bins) and ``n_total`` (the count before the ISAC_MAX_TARGETS cut); ``snapshots=True`` adds ``snapshots`` [A x n].
    Raises IsacError(INVALID_ARG) when no completed fft2D is left on the context (or a later call has rewritten its device state), IsacError(UNSUPPORTED) for a UPA."""
    lib = ctx.lib
    out = L.TargetList()
    snap = None
    if snapshots:
        dims = (C.c_int32 * 3)()
        ctx.check(lib.isac_fft2d_get_power_window(ctx.handle, None, 0, dims, None, None))
        snap = np.zeros((int(dims[2]), L.ISAC_MAX_TARGETS), dtype=np.complex128, order="F")
    ctx.check(lib.isac_fft2d_get_targets(ctx.handle, C.byref(out), None if snap is None else snap.ctypes.data_as(C.c_void_p), L.ISAC_MAX_TARGETS))
    n = int(out.n_targets)
    res = {"rng": np.array(out.rng[:n]), "vel": np.array(out.vel[:n]), "azi": np.array(out.azi[:n]), "power": np.array(out.power[:n]),
           "hits": np.array(out.hits[:n], dtype=np.int32), "row": np.array(out.row[:n], dtype=np.int32), "col": np.array(out.col[:n], dtype=np.int32),
           "n_total": int(out.n_total)}
    if snap is not None:
        res["snapshots"] = np.asfortranarray(snap[:, :n])
    return res
