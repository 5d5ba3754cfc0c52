"""sensing.estimation.refineTargets: off-grid Doppler, split-lobe merge and sidelobe flags for a target list of the last fft2D call (project-defined;
include/isac_refine.h, isac_fft2d_refine_targets)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._cpi_post import cpi_dims


def refineTargets(ctx, tl, mergeTol=0.5, mergeRows=1, sidelobeMargin=2.0, snapshots=False):
    """The entries of ``tl`` -- the dict of sensing.estimation.targetList, targetListUPA or beamDetect; anything with ``row`` and ``col`` (1-based cells of the CUT zone of
    the last completed fft2D on ``ctx``) works -- re-read off the exact periodogram of their range rows instead of the Doppler grid.

    Each cell's Doppler frequency is moved to the nearest maximum of the off-grid periodogram over all L symbols in natural order (so the two lobes that fft2D's symbol
    half-swap splits a tone into land on one frequency); an entry within ``mergeRows`` range rows and ``mergeTol`` / L cycles per symbol of an EARLIER kept entry is merged
    into it (``mergeTol=0``: nothing is merged); a kept entry that a stronger kept entry's Doppler response, times ``sidelobeMargin``, explains is flagged (``sidelobeMargin=0``: nothing is flagged).  Direction
    is scanned again on the refined snapshot, over the grids of the lists.

    Returns a dict of the KEPT entries in input order, which sensing.postProcessing.getRMSE takes as it stands: ``rng`` (the representative's grid range, as ``tl`` gives
    it; NaN when ``tl`` has no ``rng``), ``vel`` (refined), ``azi``, ``ele`` (UPA only), ``power`` (the periodogram at the refined frequency), ``row``, ``col``, ``nu``
    (cycles per symbol), ``status`` (1: the row shows no maximum near the cell -- all zero or NaN -- and the grid values stand), ``n_merged`` (entries merged into this one,
    itself included), ``sidelobe_of`` (index INTO THIS DICT of the entry that explains it, -1: none -- filter on ``sidelobe_of < 0`` for the physical targets), ``n_in``
    and, with ``snapshots=True``, ``snapshots`` [A x n_kept].
    Raises IsacError(INVALID_ARG) when no completed fft2D is left on the context, for a cell outside its CUT zone, more than ISAC_MAX_TARGETS entries or a negative or
    non-finite parameter."""
    lib = ctx.lib
    row = np.ascontiguousarray(np.asarray(tl["row"]).ravel(), dtype=np.int32)
    col = np.ascontiguousarray(np.asarray(tl["col"]).ravel(), dtype=np.int32)
    if row.size != col.size:
        raise ValueError("row and col must have one entry per cell")
    n = int(row.size)
    A = cpi_dims(ctx)[2]
    m = max(n, 1)
    status, parent, side = (np.zeros(m, dtype=np.int32) for _ in range(3))
    nu, vel, power, azi = (np.zeros(m, dtype=np.float64) for _ in range(4))
    ele = np.full(m, np.nan)
    snap = np.zeros((A, m), dtype=np.complex128, order="F") if snapshots else None
    n_kept = C.c_int32(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                           # noqa: E731
    ctx.check(lib.isac_fft2d_refine_targets(ctx.handle, p(row), p(col), n, float(mergeTol), int(mergeRows), float(sidelobeMargin), C.byref(n_kept), p(status), p(parent),
                                            p(side), p(nu), p(vel), p(power), p(azi), p(ele), None if snap is None else p(snap)))
    parent, side, status = parent[:n], side[:n], status[:n]
    kept = np.flatnonzero(parent == np.arange(n))
    assert kept.size == int(n_kept.value)
    out_of_in = np.full(n + 1, -1, dtype=np.int32)                       # input index -> output index; slot n serves sidelobe_of == -1
    out_of_in[kept] = np.arange(kept.size, dtype=np.int32)
    rng = np.asarray(tl["rng"], dtype=np.float64).ravel()[kept] if "rng" in tl else np.full(kept.size, np.nan)
    res = {"rng": rng, "vel": vel[:n][kept], "azi": azi[:n][kept], "power": power[:n][kept], "row": row[kept], "col": col[kept], "nu": nu[:n][kept],
           "status": status[kept], "n_merged": np.bincount(parent, minlength=n)[kept].astype(np.int32) if n else np.zeros(0, dtype=np.int32),
           "sidelobe_of": out_of_in[side[kept]], "n_in": n}
    if "ele" in tl or not np.isnan(ele[:n]).all():                       # the library writes ele for a planar array only
        res["ele"] = ele[:n][kept]
    if snap is not None:
        res["snapshots"] = np.asfortranarray(snap[:, :n][:, kept])
    return res
