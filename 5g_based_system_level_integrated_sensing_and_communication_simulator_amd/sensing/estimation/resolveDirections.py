"""sensing.estimation.resolveDirections: off-grid direction finding with several sources per array snapshot (project-defined; include/isac_directions.h,
isac_resolve_directions)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _lib as L
from .._marshal import est_block

_ENTRY_KEYS = ("rng", "vel", "row", "col")


def expand_rows(raw, tl, upa, twin=False):
    """The dict of resolveDirections from the raw outputs of the C call: ``raw`` maps status, n_found, n_src, residual ([n]) and azi, ele, dir_u, dir_v, power, amp
    ([max_sources x n], column-major: source k of entry i at [k, i]) to arrays.  One row per accepted source (k < n_src), entry by entry; ``rng``, ``vel``, ``row``, ``col``
    are copied from ``tl`` when it is a dict that has them.  ``twin``: the other mirror twin's degrees -- 180 - azi (ULA), (-ele, azi -+ 180) (UPA)."""
    n_src = np.asarray(raw["n_src"], dtype=np.int32)
    n = n_src.size
    entry = np.repeat(np.arange(n, dtype=np.int32), n_src)
    src = (np.arange(entry.size) - np.repeat(np.cumsum(n_src) - n_src, n_src)).astype(np.int32)
    pick = lambda a: np.asarray(a)[src, entry]                             # noqa: E731
    azi = pick(raw["azi"]).astype(np.float64)
    res = {"dir_u": pick(raw["dir_u"]), "power": pick(raw["power"]), "amp": pick(raw["amp"]), "entry": entry, "src": src}
    if upa:
        ele = pick(raw["ele"]).astype(np.float64)
        res["dir_v"] = pick(raw["dir_v"])
        if twin:
            ele, azi = -ele, np.where(azi > 0, azi - 180.0, azi + 180.0)
        res["ele"] = ele
    else:
        res["dir_v"] = np.full(entry.size, np.nan)
        if twin:
            azi = 180.0 - azi
            azi = np.where(azi > 180.0, azi - 360.0, azi)
    res["azi"] = azi
    if isinstance(tl, dict):
        for k in _ENTRY_KEYS:
            if k in tl:
                res[k] = np.asarray(tl[k]).ravel()[entry]
    for k in ("n_src", "n_found", "status", "residual"):
        res[k] = np.asarray(raw[k]).copy()
    return res


def resolveDirections(ctx, radarParams, tl, maxSources=1, cycles=16, minRatio=0.01, minPower=0.0, twin=False):
    """Up to ``maxSources`` directions per array snapshot, off the scan grid: a greedy search over the Bartlett spectrum of the residual, every maximum moved to the zero of
    the spectrum's analytic derivative, and -- from the second source on -- ``cycles`` rounds of a joint re-fit (RELAX) of all sources found so far.

    ``tl``: a complex array [A x n] (column i = entry i), or any list dict that carries ``snapshots`` -- targetList, targetListUPA, refineTargets, cleanTargets or
    beamDetect called with ``snapshots=True``.  The array type (and the UPA's nV x nH) is taken from ``radarParams`` as doaEstimation.music takes it.

    Returns a dict with one row per ACCEPTED source, entry by entry and strongest first inside an entry: ``azi``, ``ele`` (UPA only) in degrees on the principal branch
    (ULA: azi in [-90, 90]; UPA: ele in [0, 90], azi = atan2d(v, u)), ``dir_u``, ``dir_v`` (the spatial frequencies: ULA sind(azi), NaN; UPA sind(ele) cosd(azi),
    sind(ele) sind(azi)), ``power`` = |amp|^2, ``amp``, ``entry`` (index into ``tl``), ``src``; ``rng``, ``vel``, ``row``, ``col`` copied from the entry where ``tl`` has
    them, so that sensing.postProcessing.getRMSE takes the result as it stands; and per ENTRY ``n_src`` (accepted: power >= minRatio x the strongest and >= minPower),
    ``n_found``, ``status`` (1: an all-zero or NaN snapshot, nothing found) and ``residual`` (||x - sum amp a||^2 / A over all sources found).
    ``twin=True`` reports the other mirror twin's degrees (the lists report whichever twin has the lower grid index); ``dir_u`` / ``dir_v`` are the same for both.
    Raises IsacError(INVALID_ARG) for maxSources outside 1 .. min(8, A - 1), negative cycles, minRatio outside [0, 1], a negative or non-finite minPower, more than
    ISAC_MAX_TARGETS entries or a UPA whose nV x nH is not A; IsacError(UNSUPPORTED) for more than 256 elements."""
    snaps = tl["snapshots"] if isinstance(tl, dict) else tl
    x = np.asfortranarray(np.asarray(snaps, dtype=np.complex128))
    if x.ndim == 1:
        x = np.asfortranarray(x.reshape(-1, 1))
    if x.ndim != 2:
        raise ValueError("snapshots must be [A x n]")
    A, n = int(x.shape[0]), int(x.shape[1])
    ep = est_block(radarParams)
    K = int(maxSources)
    m, kk = max(n, 1), max(K, 1)
    raw = {k: np.zeros(m, dtype=np.int32) for k in ("status", "n_found", "n_src")}
    raw["residual"] = np.zeros(m)
    for k in ("azi", "ele", "dir_u", "dir_v", "power"):
        raw[k] = np.full((kk, m), np.nan, order="F")
    raw["amp"] = np.zeros((kk, m), dtype=np.complex128, order="F")
    p = lambda a: a.ctypes.data_as(C.c_void_p)                            # noqa: E731
    ctx.check(ctx.lib.isac_resolve_directions(ctx.handle, C.byref(ep), p(x) if n else None, A, n, K, int(cycles), float(minRatio), float(minPower), p(raw["status"]),
                                              p(raw["n_found"]), p(raw["n_src"]), p(raw["azi"]), p(raw["ele"]), p(raw["dir_u"]), p(raw["dir_v"]), p(raw["power"]),
                                              p(raw["amp"]), p(raw["residual"])))
    raw = {k: (v[:n] if v.ndim == 1 else v[:, :n]) for k, v in raw.items()}
    return expand_rows(raw, tl, bool(ep.array_is_upa), twin)
