"""sensing.estimation.refineRange: off-grid range of the entries of a target list, from the two grids of the CPI (project-defined; include/isac_subsample.h,
isac_range_refine_dev)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _lib as L
from .._marshal import est_block


def range_refine(ctx, rxGrid, txGrid, radarParams, row, nu, probeOnly=False):
    """isac_range_refine_dev on flat arrays: (status, rho, rng, power, snapshots [A x n]) for the 1-based rdm rows ``row`` and the Doppler frequencies ``nu`` (cycles per
    symbol).  ``rxGrid`` / ``txGrid``: [K x L x A], DeviceArrays or NumPy arrays (uploaded for the call)."""
    d_rx = rxGrid if isinstance(rxGrid, L.DeviceArray) else ctx.to_device(L.as_c128_f(rxGrid))
    d_tx = txGrid if isinstance(txGrid, L.DeviceArray) else ctx.to_device(L.as_c128_f(txGrid))
    if tuple(d_rx.shape) != tuple(d_tx.shape) or len(d_rx.shape) not in (2, 3):
        raise ValueError("rxGrid and txGrid must both be [K x L x A]")
    K, Ls = int(d_rx.shape[0]), int(d_rx.shape[1])
    A = int(d_rx.shape[2]) if len(d_rx.shape) == 3 else 1
    row = np.ascontiguousarray(np.asarray(row).ravel(), dtype=np.int32)
    nu = L.as_f64(nu)
    if row.size != nu.size:
        raise ValueError("row and nu must have one entry per target")
    n = int(row.size)
    m = max(n, 1)
    status = np.zeros(m, dtype=np.int32)
    rho, rng, power = (np.zeros(m, dtype=np.float64) for _ in range(3))
    snap = np.zeros((A, m), dtype=np.complex128, order="F")
    ep = est_block(radarParams)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                           # noqa: E731
    ctx.check(ctx.lib.isac_range_refine_dev(ctx.handle, C.byref(ep), d_rx, d_tx, K, Ls, A, p(row), p(nu), n, 1 if probeOnly else 0, p(status), p(rho), p(rng), p(power),
                                            p(snap)))
    return status[:n], rho[:n], rng[:n], power[:n], np.asfortranarray(snap[:, :n])


def refineRange(ctx, rxGrid, txGrid, radarParams, tl):
    """The ranges of ``tl`` -- the dict of sensing.estimation.targetList, targetListUPA, beamDetect, refineTargets, cleanTargets or relaxTargets; anything with ``row``
    (1-based rdm rows) and either ``nu`` (cycles per symbol) or ``col`` (1-based rdm columns: nu = (col - nFFT/2 - 1) / nFFT) works -- re-read off the exact delay
    periodogram of ``rxGrid .* conj(txGrid)`` at each entry's Doppler frequency instead of the range grid: the maximum within one bin of the entry's row.  ``rxGrid`` /
    ``txGrid``: the grids fft2D took, [K x L x A], DeviceArrays or NumPy arrays.  ULA and UPA alike; direction is not scanned again: sensing.estimation.resolveDirections
    takes ``range_snapshots``.

    Returns a copy of ``tl``, which sensing.postProcessing.getRMSE takes as it stands, with ``rng`` replaced by the refined range and, per entry, ``rho`` (the 0-based
    continuous range bin, rng = rho rRes), ``rng_grid`` ((row - 1) rRes), ``range_power`` (the periodogram at rho), ``range_status`` (1: no maximum within one bin of the
    row -- an empty row -- and the grid range stands) and ``range_snapshots`` [A x n] (the array snapshot at (rho, nu), without the range-axis weight of a bin).
    Raises IsacError(INVALID_ARG) for a row outside 1 .. nIFFT, a non-finite nu or more than ISAC_MAX_TARGETS entries."""
    row = np.ascontiguousarray(np.asarray(tl["row"]).ravel(), dtype=np.int32)
    if "nu" in tl:
        nu = L.as_f64(tl["nu"])
    else:
        n_fft = int(radarParams.nFFT)
        nu = (np.asarray(tl["col"], dtype=np.float64).ravel() - n_fft // 2 - 1) / n_fft
    status, rho, rng, power, snap = range_refine(ctx, rxGrid, txGrid, radarParams, row, nu)
    res = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in tl.items()}
    res.update(rng=rng, rho=rho, rng_grid=(row - 1) * float(radarParams.rRes), range_power=power, range_status=status, range_snapshots=snap)
    return res
