"""sensing.estimation.beamClean: successive target cancellation (CLEAN) with the detector on beam planes of the last fft2D call (project-defined;
include/isac_beam_clean.h, isac_fft2d_beam_clean_targets)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _lib as L
from ..detection.cfarDetect import method_block
from ._cpi_post import add_optional, cpi_dims, kept_entries, ptr as p, symbol_count, symbol_mask


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
    nr, nc, A = cpi_dims(ctx)
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
    act = symbol_mask(symActive)
    n_sym = symbol_count(ctx, A, nSymbols, act, residual)
    snap = np.zeros((A, cap), dtype=np.complex128, order="F") if snapshots else None
    res_rows = np.zeros((nr, n_sym, A), dtype=np.complex128, order="F") if residual else None
    bp = np.zeros((nr, nc, min(B, L.ISAC_MAX_BEAMS)), dtype=np.float64, order="F") if beamPow else None   # (more beams than that: the library refuses the call)
    left = np.zeros((L.ISAC_MAX_TARGETS, 2), dtype=np.int32)              # [2 x ISAC_MAX_TARGETS] column-major = one (row, col) pair per C row
    n_iter, n_kept, n_left = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    ctx.check(lib.isac_fft2d_beam_clean_targets(ctx.handle, p(w), B, p(lab), C.byref(m), n_max, int(spanRows), float(mergeTol), p(act), C.byref(n_iter), C.byref(n_kept),
                                                C.byref(n_left), p(row), p(col), p(hits), p(beam), p(status), p(parent), p(map_power), p(nu), p(vel), p(rng), p(power), p(azi),
                                                p(ele), p(beam_label), p(snap), p(res_rows), p(bp), p(left)))
    n = int(n_iter.value)
    res, kept = kept_entries(n, int(n_kept.value), int(n_left.value), dict(rng=rng, vel=vel, azi=azi, power=power, hits=hits, row=row, col=col, nu=nu, status=status,
                                                                           parent=parent, map_power=map_power))
    res.update({"beam": beam[:n][kept], "beam_label": beam_label[:n][kept], "left_cells": left[:min(int(n_left.value), L.ISAC_MAX_TARGETS)].copy()})
    add_optional(res, ctx, ele, n, kept, snap, res_rows)
    if bp is not None:
        res["beam_pow"] = bp
    return res
