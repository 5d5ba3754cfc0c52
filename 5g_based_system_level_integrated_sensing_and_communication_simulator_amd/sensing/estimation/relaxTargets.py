"""sensing.estimation.relaxTargets: joint re-fit (RELAX) of the Doppler tones of a target list on the range rows of the last fft2D call (project-defined;
include/isac_relax.h, isac_fft2d_relax_targets)."""
from __future__ import annotations

import numpy as np

from ._cpi_post import add_optional, cpi_dims, ptr as p, symbol_count, symbol_mask


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
    nr, _, A = cpi_dims(ctx)
    cap = max(n, 1)
    status = np.zeros(cap, dtype=np.int32)
    nu, vel, power, shift, last_step, azi = (np.zeros(cap, dtype=np.float64) for _ in range(6))
    ele = np.full(cap, np.nan)
    act = symbol_mask(symActive)
    snap = np.zeros((A, cap), dtype=np.complex128, order="F") if snapshots else None
    n_sym = symbol_count(ctx, A, nSymbols, act, residual)
    res_rows = np.zeros((nr, n_sym, A), dtype=np.complex128, order="F") if residual else None
    ctx.check(lib.isac_fft2d_relax_targets(ctx.handle, p(row), p(nu_in), n, int(cycles), int(spanRows), float(box), p(act), p(status), p(nu), p(vel), p(power), p(shift),
                                           p(last_step), p(azi), p(ele), p(snap), p(res_rows)))
    rng = get("rng")
    res = {"rng": np.full(n, np.nan) if rng is None else np.array(np.asarray(rng).ravel(), dtype=np.float64), "vel": vel[:n], "azi": azi[:n], "power": power[:n], "row": row,
           "nu": nu[:n], "status": status[:n], "shift": shift[:n], "last_step": last_step[:n]}
    if get("col") is not None:
        res["col"] = np.array(np.asarray(get("col")).ravel(), dtype=np.int32)
    add_optional(res, ctx, ele, n, slice(None), snap, res_rows)
    return res
