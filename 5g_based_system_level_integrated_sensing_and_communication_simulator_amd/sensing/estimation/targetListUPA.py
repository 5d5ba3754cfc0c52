"""sensing.estimation.targetListUPA: the per-target list of the last fft2D call on a uniform planar array (project-defined; include/isac_targets_upa.h,
isac_fft2d_get_targets_upa)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _lib as L


def targetListUPA(ctx, snapshots=False):
    """Paired (range, velocity, azimuth, elevation) entries of the last completed fft2D on ``ctx`` (a UPA CPI), strongest first.

    The cells, their order, ``rng`` and ``vel`` are those of sensing.estimation.targetList -- that part does not know the array type; each cell's array snapshot is then
    scanned over the elevation x azimuth grid of the UPA DoA (Bartlett, the steering vector of music.m:44-55) and the first arg-max gives ``azi`` and ``ele``.  Returns the
    dict of targetList -- ``rng, vel, azi, power, hits, row, col`` (1-based bins), ``n_total``, with ``snapshots=True`` also ``snapshots`` [A x n] -- plus ``ele``.
    It does not need ``ctx.set_upa_doa(True)``: a UPA fft2D that raised IsacError(UNSUPPORTED) for its own DoA stage has still left what the list is made of.
    Raises IsacError(INVALID_ARG) when no completed fft2D is left on the context (or a later call has rewritten its device state) or nV x nH is not the antenna count,
    IsacError(UNSUPPORTED) for a ULA (use targetList) and for more than 256 elements."""
    lib = ctx.lib
    out = L.TargetList()
    ele = (C.c_double * L.ISAC_MAX_TARGETS)()
    snap = None
    if snapshots:
        dims = (C.c_int32 * 3)()
        ctx.check(lib.isac_fft2d_get_power_window(ctx.handle, None, 0, dims, None, None))
        snap = np.zeros((int(dims[2]), L.ISAC_MAX_TARGETS), dtype=np.complex128, order="F")
    ctx.check(lib.isac_fft2d_get_targets_upa(ctx.handle, C.byref(out), ele, None if snap is None else snap.ctypes.data_as(C.c_void_p), L.ISAC_MAX_TARGETS))
    n = int(out.n_targets)
    res = {"rng": np.array(out.rng[:n]), "vel": np.array(out.vel[:n]), "azi": np.array(out.azi[:n]), "ele": np.array(ele[:n]), "power": np.array(out.power[:n]),
           "hits": np.array(out.hits[:n], dtype=np.int32), "row": np.array(out.row[:n], dtype=np.int32), "col": np.array(out.col[:n], dtype=np.int32),
           "n_total": int(out.n_total)}
    if snap is not None:
        res["snapshots"] = np.asfortranarray(snap[:, :n])
    return res
