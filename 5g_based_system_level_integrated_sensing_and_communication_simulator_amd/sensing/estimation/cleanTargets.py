"""sensing.estimation.cleanTargets: successive target cancellation (CLEAN) on the range rows of the last fft2D call (project-defined; include/isac_clean.h,
isac_fft2d_clean_targets)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _lib as L
from ..detection.cfarDetect import method_block


def cleanTargets(ctx, maxIter=16, spanRows=2, mergeTol=0.5, Method="CA", Rank=1, ThresholdFactor="Auto", CustomThresholdFactor=None, symActive=None, snapshots=False,
                 residual=False, nSymbols=None):
    """The targets of the last completed fft2D on ``ctx`` by successive cancellation: detect (detector ``Method`` -- 'CA', 'GOCA', 'SOCA', 'OS' with ``Rank``;
    ``ThresholdFactor`` 'Auto' or 'Custom', as sensing.estimation.redetect and beamDetect take them) on a copy of the CPI's range rows, take the strongest listed cell,
    estimate its Doppler tone off the grid (the refinement of sensing.estimation.refineTargets), subtract the tone from the range rows within ``spanRows`` rows of the cell,
    and detect again on what is left -- at most ``maxIter`` times.  A target hidden under a stronger one's Doppler sidelobes appears once the stronger one is gone; the
    sidelobes, split lobes and gap lobes of a tone go with it instead of being listed.

    ``symActive`` [L]: truthy where the symbol was transmitted (None: all).  With a silent 'S' slot in the CPI, name it: a tone fitted across the gap leaves a residue that
    masks what the pass was meant to uncover.  An entry within ``spanRows`` rows and ``mergeTol`` / L cycles per symbol of an EARLIER kept entry is a residue of an
    imperfect subtraction and is left out (``mergeTol=0``: every entry is kept).

    THE SYMBOL COUNT L.  The library reads ``symActive`` and writes ``residual`` by the L of the CPI and takes the caller's arrays on trust; the C ABI has no getter for L.
    sensing.estimation.fft2D / fft2D_submit record the grid shape on ``ctx`` and this function sizes and checks both arrays by it.  After any other route to a CPI
    (sensing.submitN, the C entry points called directly) pass ``nSymbols`` yourself whenever ``symActive`` or ``residual`` is used -- a wrong value there is an
    out-of-bounds access; a value that contradicts the recorded shape raises ValueError.

    Returns a dict of the KEPT entries in the order they were extracted, which sensing.postProcessing.getRMSE takes as it stands: the keys of
    sensing.estimation.targetList -- ``rng``, ``vel`` (refined), ``azi``, ``ele`` (UPA only), ``power`` (the periodogram at the refined frequency), ``hits``, ``row``,
    ``col``, ``n_total`` (entries extracted, residues included) -- plus ``nu`` (cycles per symbol), ``status`` (1: the row showed no maximum near the cell; the loop stopped
    there), ``parent`` (index into this dict: every kept entry is its own), ``n_merged`` (residues left out in favour of this entry, itself included), ``map_power`` (the
    summed map at the cell when it was picked), ``n_left`` (cells still listed after the last pass: 0 = the map is exhausted) and, on request, ``snapshots``
    [A x n_kept] and ``residual`` [nr x L x A] (the window's range rows after the last subtraction).
    Raises IsacError(INVALID_ARG) when no completed fft2D is left on the context or for a parameter out of range, IsacError(UNSUPPORTED) for a CFAR halo of 0."""
    lib = ctx.lib
    m = method_block(Method, Rank, ThresholdFactor, CustomThresholdFactor)
    n_max = int(maxIter)
    dims = (C.c_int32 * 3)()
    ctx.check(lib.isac_fft2d_get_power_window(ctx.handle, None, 0, dims, None, None))
    nr, A = int(dims[0]), int(dims[2])
    cap = min(max(n_max, 1), L.ISAC_MAX_TARGETS)
    row, col, hits, status, parent = (np.zeros(cap, dtype=np.int32) for _ in range(5))
    map_power, nu, vel, rng, power, azi = (np.zeros(cap, dtype=np.float64) for _ in range(6))
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
    n_iter, n_kept, n_left = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)     # noqa: E731
    ctx.check(lib.isac_fft2d_clean_targets(ctx.handle, C.byref(m), n_max, int(spanRows), float(mergeTol), p(act), C.byref(n_iter), C.byref(n_kept), C.byref(n_left), p(row), p(col),
                                           p(hits), p(status), p(parent), p(map_power), p(nu), p(vel), p(rng), p(power), p(azi), p(ele), p(snap), p(res_rows)))
    n = int(n_iter.value)
    parent = parent[:n]
    kept = np.flatnonzero(parent == np.arange(n))
    assert kept.size == int(n_kept.value)
    out_of_in = np.full(n, -1, dtype=np.int32)
    out_of_in[kept] = np.arange(kept.size, dtype=np.int32)
    res = {"rng": rng[:n][kept], "vel": vel[:n][kept], "azi": azi[:n][kept], "power": power[:n][kept], "hits": hits[:n][kept], "row": row[:n][kept], "col": col[:n][kept],
           "n_total": n, "nu": nu[:n][kept], "status": status[:n][kept], "parent": out_of_in[parent[kept]],
           "n_merged": np.bincount(parent, minlength=n)[kept].astype(np.int32) if n else np.zeros(0, dtype=np.int32), "map_power": map_power[:n][kept],
           "n_left": int(n_left.value)}
    rp = getattr(ctx, "fft2d_radar_params", None)                          # the array type, where the context knows it; else: the library writes ele for a planar array only
    kind = getattr(rp.get("antennaType") if isinstance(rp, dict) else getattr(rp, "antennaType", None), "kind", None)
    upa = kind == "upa" if rp is not None else not np.isnan(ele[:n]).all()
    if upa:
        res["ele"] = ele[:n][kept]
    if snap is not None:
        res["snapshots"] = np.asfortranarray(snap[:, :n][:, kept])
    if res_rows is not None:
        res["residual"] = res_rows
    return res
