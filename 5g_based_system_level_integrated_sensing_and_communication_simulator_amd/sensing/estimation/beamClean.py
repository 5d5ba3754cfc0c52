"""sensing.estimation.beamClean: successive target cancellation (CLEAN) with the detector on beam planes of the last fft2D call (project-defined;
include/isac_beam_clean.h, isac_fft2d_beam_clean_targets)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _lib as L
from ..detection.cfarDetect import method_block


def beamClean(ctx, W, beam_azi=None, maxIter=16, spanRows=2, mergeTol=0.5, Method="CA", Rank=1, ThresholdFactor="Auto", CustomThresholdFactor=None, symActive=None,
              snapshots=False, residual=False, beamPow=False, nSymbols=None):
    """The targets of the last completed fft2D on ``ctx`` by successive cancellation with the array combined coherently BEFORE the detector: the loop of
    sensing.estimation.cleanTargets with the detection of sensing.estimation.beamDetect.  Every pass weights the complex range-Doppler window of the residual range rows by
    the columns of ``W`` [A x B] (sensing.estimation.beamWeights gives matched columns), runs detector ``Method`` ('CA', 'GOCA', 'SOCA', 'OS' with ``Rank``;
    ``ThresholdFactor`` 'Auto' or 'Custom') on every beam plane, takes the strongest listed cell of the map "strongest beam per cell", estimates its Doppler tone off the grid
    (the refinement of sensing.estimation.refineTargets, all elements summed), subtracts the tone from the range rows within ``spanRows`` rows of the cell, and detects again
    -- at most ``maxIter`` times.  An echo that no single element lifts over its threshold AND that lies under a stronger echo's Doppler sidelobes is found by neither
    cleanTargets nor beamDetect; it is found here.  The library keeps the planes on the device and forms only the rows a subtraction changed again.

    ``beam_azi`` [B]: a label per column of W (None: the beam number).  ``symActive``, ``mergeTol``, ``nSymbols``: as sensing.estimation.cleanTargets takes them (the symbol
    count L is read from the grid shape sensing.estimation.fft2D recorded on ``ctx``; after any other route to a CPI pass ``nSymbols`` whenever ``symActive`` or ``residual``
    is used -- a wrong value there is an out-of-bounds access).

    Returns the dict of sensing.estimation.cleanTargets -- the KEPT entries in the order they were extracted: ``rng``, ``vel`` (refined), ``azi`` (the Bartlett scan of the
    refined snapshot), ``ele`` (UPA only), ``power``, ``hits`` (beams that detect the cell), ``row``, ``col``, ``n_total``, ``nu``, ``status``, ``parent``, ``n_merged``,
    ``map_power`` (the strongest beam's power at the cell when it was picked), ``n_left`` -- plus ``beam`` (1-based column of W with that maximum), ``beam_label``
    (``beam_azi[beam - 1]``, or the beam number) and ``left_cells`` [n x 2]: the (row, col) pairs still listed after the last pass (at most ISAC_MAX_TARGETS of the
    ``n_left``).  On request ``snapshots`` [A x n_kept], ``residual`` [nr x L x A] and ``beam_pow`` [nr x nc x B] (the planes the last pass saw).
    sensing.estimation.refineTargets, relaxTargets, resolveDirections and sensing.postProcessing.getRMSE take the result as they take cleanTargets'.
    Raises IsacError(INVALID_ARG) when no completed fft2D is left on the context or for a parameter out of range, IsacError(UNSUPPORTED) for a CFAR halo of 0 or more than
    ISAC_MAX_BEAMS beams, ValueError for arrays whose shapes contradict the CPI."""
    lib = ctx.lib
    m = method_block(Method, Rank, ThresholdFactor, CustomThresholdFactor)
    n_max = int(maxIter)
    dims = (C.c_int32 * 3)()
    ctx.check(lib.isac_fft2d_get_power_window(ctx.handle, None, 0, dims, None, None))
    nr, nc, A = int(dims[0]), int(dims[1]), int(dims[2])
    w = L.as_c128_f(W)
    if w.ndim != 2 or w.shape[0] != A:
        raise ValueError(f"W must be [A x B] with A = {A}")
    B = w.shape[1]
    lab = None
    if beam_azi is not None:
        lab = L.as_f64(beam_azi)
        if lab.size != B:
            raise ValueError("beam_azi needs one label per column of W")
    cap = min(max(n_max, 1), L.ISAC_MAX_TARGETS)
    row, col, hits, beam, status, parent = (np.zeros(cap, dtype=np.int32) for _ in range(6))
    map_power, nu, vel, rng, power, azi, beam_label = (np.zeros(cap, dtype=np.float64) for _ in range(7))
    ele = np.full(cap, np.nan)
    act = None
    if symActive is not None:
        act = np.ascontiguousarray(np.asarray(symActive).ravel() != 0, dtype=np.uint8)
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
    snap = np.zeros((A, cap), dtype=np.complex128, order="F") if snapshots else None
    res_rows = np.zeros((nr, n_sym, A), dtype=np.complex128, order="F") if residual else None
    bp = np.zeros((nr, nc, min(B, L.ISAC_MAX_BEAMS)), dtype=np.float64, order="F") if beamPow else None   # (more beams than that: the library refuses the call)
    left = np.zeros((L.ISAC_MAX_TARGETS, 2), dtype=np.int32)              # [2 x ISAC_MAX_TARGETS] column-major = one (row, col) pair per C row
    n_iter, n_kept, n_left = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)     # noqa: E731
    ctx.check(lib.isac_fft2d_beam_clean_targets(ctx.handle, p(w), B, p(lab), C.byref(m), n_max, int(spanRows), float(mergeTol), p(act), C.byref(n_iter), C.byref(n_kept),
                                                C.byref(n_left), p(row), p(col), p(hits), p(beam), p(status), p(parent), p(map_power), p(nu), p(vel), p(rng), p(power), p(azi),
                                                p(ele), p(beam_label), p(snap), p(res_rows), p(bp), p(left)))
    n = int(n_iter.value)
    parent = parent[:n]
    kept = np.flatnonzero(parent == np.arange(n))
    assert kept.size == int(n_kept.value)
    out_of_in = np.full(n, -1, dtype=np.int32)
    out_of_in[kept] = np.arange(kept.size, dtype=np.int32)
    res = {"rng": rng[:n][kept], "vel": vel[:n][kept], "azi": azi[:n][kept], "power": power[:n][kept], "hits": hits[:n][kept], "row": row[:n][kept], "col": col[:n][kept],
           "n_total": n, "nu": nu[:n][kept], "status": status[:n][kept], "parent": out_of_in[parent[kept]],
           "n_merged": np.bincount(parent, minlength=n)[kept].astype(np.int32) if n else np.zeros(0, dtype=np.int32), "map_power": map_power[:n][kept],
           "n_left": int(n_left.value), "beam": beam[:n][kept], "beam_label": beam_label[:n][kept],
           "left_cells": left[:min(int(n_left.value), L.ISAC_MAX_TARGETS)].copy()}
    rp = getattr(ctx, "fft2d_radar_params", None)                          # the array type, where the context knows it; else: the library writes ele for a planar array only
    kind = getattr(rp.get("antennaType") if isinstance(rp, dict) else getattr(rp, "antennaType", None), "kind", None)
    upa = kind == "upa" if rp is not None else not np.isnan(ele[:n]).all()
    if upa:
        res["ele"] = ele[:n][kept]
    if snap is not None:
        res["snapshots"] = np.asfortranarray(snap[:, :n][:, kept])
    if res_rows is not None:
        res["residual"] = res_rows
    if bp is not None:
        res["beam_pow"] = bp
    return res
