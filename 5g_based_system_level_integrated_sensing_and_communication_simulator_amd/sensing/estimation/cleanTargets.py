"""sensing.estimation.cleanTargets: successive target cancellation (CLEAN) on the range rows of the last fft2D call (project-defined; include/isac_clean.h,
isac_fft2d_clean_targets)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _lib as L
from ..detection.cfarDetect import method_block
from ._cpi_post import add_optional, cpi_dims, kept_entries, ptr as p, symbol_count, symbol_mask


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
    nr, _, A = cpi_dims(ctx)
    cap = min(max(n_max, 1), L.ISAC_MAX_TARGETS)
    row, col, hits, status, parent = (np.zeros(cap, dtype=np.int32) for _ in range(5))
    map_power, nu, vel, rng, power, azi = (np.zeros(cap, dtype=np.float64) for _ in range(6))
    ele = np.full(cap, np.nan)
    act = symbol_mask(symActive)
    snap = np.zeros((A, cap), dtype=np.complex128, order="F") if snapshots else None
    n_sym = symbol_count(ctx, A, nSymbols, act, residual)
    res_rows = np.zeros((nr, n_sym, A), dtype=np.complex128, order="F") if residual else None
    n_iter, n_kept, n_left = C.c_int32(0), C.c_int32(0), C.c_int32(0)
    ctx.check(lib.isac_fft2d_clean_targets(ctx.handle, C.byref(m), n_max, int(spanRows), float(mergeTol), p(act), C.byref(n_iter), C.byref(n_kept), C.byref(n_left), p(row), p(col),
                                           p(hits), p(status), p(parent), p(map_power), p(nu), p(vel), p(rng), p(power), p(azi), p(ele), p(snap), p(res_rows)))
    n = int(n_iter.value)
    res, kept = kept_entries(n, int(n_kept.value), int(n_left.value), dict(rng=rng, vel=vel, azi=azi, power=power, hits=hits, row=row, col=col, nu=nu, status=status,
                                                                           parent=parent, map_power=map_power))
    add_optional(res, ctx, ele, n, kept, snap, res_rows)
    return res
