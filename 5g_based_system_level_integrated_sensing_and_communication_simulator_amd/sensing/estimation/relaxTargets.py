"""sensing.estimation.relaxTargets: joint re-fit (RELAX) of the Doppler tones of a target list on the range rows of the last fft2D call (project-defined;
include/isac_relax.h, isac_fft2d_relax_targets)."""
from __future__ import annotations

import ctypes as C

import numpy as np


def relaxTargets(ctx, cl, cycles=16, spanRows=2, box=0.5, symActive=None, snapshots=False, residual=False, nSymbols=None):
    """The entries of ``cl`` -- the dict of sensing.estimation.cleanTargets or refineTargets, or anything with ``row`` (1-based range rows) and ``nu`` (cycles per symbol) --
    re-fitted jointly on a copy of the range rows of the last completed fft2D on ``ctx``: every tone is subtracted from the rows within ``spanRows`` rows of its own; then,
    ``cycles`` times and entry after entry, one tone is put back, its frequency is searched again within ``box`` / L of where it stood, and it is fitted and subtracted
    again.  Two targets that share a range row and lie one to three Doppler lobes apart bias each other's frequency in a sequential extraction; the re-fit removes that
    bias (not the noise).  No entry is added, dropped or merged.

    ``symActive`` [L] and the symbol count ``nSymbols``: as sensing.estimation.cleanTargets takes them -- the library reads ``symActive`` and writes ``residual`` by the L
    of the CPI and takes the caller's arrays on trust; sensing.estimation.fft2D / fft2D_submit record the grid shape on ``ctx``, after any other route to a CPI pass
    ``nSymbols`` whenever ``symActive`` or ``residual`` is used.

    Returns a dict, in input order, which sensing.postProcessing.getRMSE takes as it stands: ``rng`` (the input's; without one NaN), ``vel`` (nu nFFT vRes), ``azi``,
    ``ele`` (UPA only), ``power`` (the periodogram of the restored tone at its frequency), ``row``, ``col`` (the input's, if any), ``nu``, ``status`` (1: the last cycle's
    search found no maximum inside the box and the entry stood), ``shift`` (|nu - nu_in| L), ``last_step`` (the last cycle's move, in units of 1 / L: how far the re-fit is
    from converged) and, on request, ``snapshots`` [A x n] and ``residual`` [nr x L x A] (the window's range rows with every tone subtracted).
    Raises IsacError(INVALID_ARG) when no completed fft2D is left on the context or for a parameter out of range."""
    lib = ctx.lib
    get = cl.get if isinstance(cl, dict) else lambda k, d=None: getattr(cl, k, d)   # noqa: E731
    row = np.ascontiguousarray(np.asarray(get("row")).ravel(), dtype=np.int32)
    nu_in = np.ascontiguousarray(np.asarray(get("nu")).ravel(), dtype=np.float64)
    if row.size != nu_in.size:
        raise ValueError("row and nu need one entry per target")
    n = int(row.size)
    dims = (C.c_int32 * 3)()
    ctx.check(lib.isac_fft2d_get_power_window(ctx.handle, None, 0, dims, None, None))
    nr, A = int(dims[0]), int(dims[2])
    cap = max(n, 1)
    status = np.zeros(cap, dtype=np.int32)
    nu, vel, power, shift, last_step, azi = (np.zeros(cap, dtype=np.float64) for _ in range(6))
    ele = np.full(cap, np.nan)
    act = None
    if symActive is not None:
        act = np.ascontiguousarray(np.asarray(symActive).ravel() != 0, dtype=np.uint8)
    snap = np.zeros((A, cap), dtype=np.complex128, order="F") if snapshots else None
    res_rows = None
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
    if residual:
        res_rows = np.zeros((nr, n_sym, A), dtype=np.complex128, order="F")
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)     # noqa: E731
    ctx.check(lib.isac_fft2d_relax_targets(ctx.handle, p(row), p(nu_in), n, int(cycles), int(spanRows), float(box), p(act), p(status), p(nu), p(vel), p(power), p(shift),
                                           p(last_step), p(azi), p(ele), p(snap), p(res_rows)))
    rng = get("rng")
    res = {"rng": np.full(n, np.nan) if rng is None else np.array(np.asarray(rng).ravel(), dtype=np.float64), "vel": vel[:n], "azi": azi[:n], "power": power[:n], "row": row,
           "nu": nu[:n], "status": status[:n], "shift": shift[:n], "last_step": last_step[:n]}
    if get("col") is not None:
        res["col"] = np.array(np.asarray(get("col")).ravel(), dtype=np.int32)
    rp = getattr(ctx, "fft2d_radar_params", None)                          # the array type, where the context knows it; else: the library writes ele for a planar array only
    kind = getattr(rp.get("antennaType") if isinstance(rp, dict) else getattr(rp, "antennaType", None), "kind", None)
    upa = kind == "upa" if rp is not None else not np.isnan(ele[:n]).all()
    if upa:
        res["ele"] = ele[:n]
    if snap is not None:
        res["snapshots"] = np.asfortranarray(snap[:, :n])
    if res_rows is not None:
        res["residual"] = res_rows
    return res
