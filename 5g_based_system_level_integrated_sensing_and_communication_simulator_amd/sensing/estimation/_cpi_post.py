"""What the wrappers of the calls on "the last completed fft2D" share (cleanTargets, beamClean, relaxTargets, refineTargets, redetect): the CPI's dimensions, its symbol
count, the symbol mask, the array-type probe and the dict of kept entries.  Private to sensing.estimation."""
from __future__ import annotations

import ctypes as C

import numpy as np


def cpi_dims(ctx):
    """(nr, nc, A) of the power window of the last completed fft2D on ``ctx``; IsacError(INVALID_ARG) when there is none."""
    dims = (C.c_int32 * 3)()
    ctx.check(ctx.lib.isac_fft2d_get_power_window(ctx.handle, None, 0, dims, None, None))
    return int(dims[0]), int(dims[1]), int(dims[2])


def symbol_mask(symActive):
    """``symActive`` as the uint8 array the library reads, or None."""
    if symActive is None:
        return None
    return np.ascontiguousarray(np.asarray(symActive).ravel() != 0, dtype=np.uint8)


def symbol_count(ctx, A, nSymbols, act, residual):
    """The symbol count L of the CPI -- the grid shape sensing.estimation.fft2D / fft2D_submit recorded on ``ctx``, or the caller's ``nSymbols`` -- or None where nothing
    needs it.  ValueError: ``nSymbols`` contradicts the recorded shape, the mask ``act`` or ``residual`` is asked for without a count, or ``act`` has another length."""
    shape = getattr(ctx, "fft2d_grid_shape", None)                         # (K, L, A) of the last sensing.estimation.fft2D / fft2D_submit on this context
    n_sym = int(shape[1]) if shape is not None and int(shape[2]) == A else None
    if nSymbols is not None:
        if n_sym is not None and int(nSymbols) != n_sym:
            raise ValueError(f"nSymbols = {int(nSymbols)}, but the CPI on this context has {n_sym} symbols")
        n_sym = int(nSymbols)
    if (act is not None or residual) and n_sym is None:
        raise ValueError("symActive and residual need the CPI's symbol count: this context ran no sensing.estimation.fft2D, pass nSymbols")
    if act is not None and act.size != n_sym:
        raise ValueError(f"symActive needs one entry per symbol of the CPI ({n_sym})")
    return n_sym


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def kept_entries(n, n_kept, n_left, out):
    """The dict of sensing.estimation.cleanTargets from the library's per-entry arrays ``out`` (name -> array) after ``n`` entries, and the indices of the kept ones."""
    parent = out["parent"][:n]
    kept = np.flatnonzero(parent == np.arange(n))
    assert kept.size == n_kept
    out_of_in = np.full(n, -1, dtype=np.int32)
    out_of_in[kept] = np.arange(kept.size, dtype=np.int32)
    res = {k: out[k][:n][kept] for k in ("rng", "vel", "azi", "power", "hits", "row", "col")}
    res.update({"n_total": n, "nu": out["nu"][:n][kept], "status": out["status"][:n][kept], "parent": out_of_in[parent[kept]],
                "n_merged": np.bincount(parent, minlength=n)[kept].astype(np.int32) if n else np.zeros(0, dtype=np.int32), "map_power": out["map_power"][:n][kept],
                "n_left": n_left})
    return res, kept


def add_optional(res, ctx, ele, n, kept, snap, res_rows):
    """``ele`` (UPA only), ``snapshots`` and ``residual`` of the entries ``kept`` (indices, or slice(None)) into ``res``."""
    rp = getattr(ctx, "fft2d_radar_params", None)                          # the array type, where the context knows it; else: the library writes ele for a planar array only
    kind = getattr(rp.get("antennaType") if isinstance(rp, dict) else getattr(rp, "antennaType", None), "kind", None)
    upa = kind == "upa" if rp is not None else not np.isnan(ele[:n]).all()
    if upa:
        res["ele"] = ele[:n][kept]
    if snap is not None:
        res["snapshots"] = np.asfortranarray(snap[:, :n][:, kept])
    if res_rows is not None:
        res["residual"] = res_rows
