"""sensing.postProcessing.getPositionRMSE: position error of sensing.estimation.localizeTargets' estimates (host; project-defined, in getRMSE's style)."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np


def getPositionRMSE(est, truthPositions, gate):
    """Per estimate, in order: the horizontal distance to the nearest truth position no earlier estimate has been matched to, if it is within ``gate`` metres (strict, as
    getRMSE's range test), else NaN; a matched truth is taken.  ``est``: the dict of localizeTargets (``pos`` [n x 2]) or an [n x 2] array; ``truthPositions`` [Q x 2] or
    [Q x 3] (x, y used).  Returns a namespace of ``posRMSE`` [n] and ``match`` [n] (the truth's index, or -1); ``float('nan')`` when there is no estimate (getRMSE.m:31-35)."""
    pos = np.asarray(est["pos"] if isinstance(est, dict) else est, dtype=np.float64).reshape(-1, 2)
    truth = np.asarray(truthPositions, dtype=np.float64)
    truth = truth.reshape(-1, truth.shape[-1] if truth.ndim > 1 else 2)[:, :2]
    if pos.shape[0] == 0:
        return float("nan")
    err, match = np.full(pos.shape[0], math.nan), np.full(pos.shape[0], -1, dtype=np.int64)
    free = np.ones(truth.shape[0], dtype=bool)
    for i, p in enumerate(pos):
        d = np.where(free, np.hypot(truth[:, 0] - p[0], truth[:, 1] - p[1]), np.inf)
        if d.size and np.isfinite(d).any():
            j = int(np.argmin(d))                                            # the first of equal distances
            if d[j] < gate:
                err[i], match[i], free[j] = d[j], j, False
    return SimpleNamespace(posRMSE=err, match=match)
