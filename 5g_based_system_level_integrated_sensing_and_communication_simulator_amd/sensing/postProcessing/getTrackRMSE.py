"""sensing.postProcessing.getTrackRMSE: errors, id switches and false tracks of a sensing.estimation.trackTargets history against truth trajectories (host; project-defined,
in getPositionRMSE's style)."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np


def getTrackRMSE(history, truth, gate, bank=0):
    """``history``: the list trackTargets returns (per scan a dict whose ``tracks[bank]`` holds ``id, status, x``).  ``truth`` [S x Q x 4] (x, y, vx, vy of truth target q
    at scan s) or [S x Q x 2] (positions only: velRMSE is NaN).  In every scan the confirmed tracks, in slot order, are matched as getPositionRMSE matches estimates: a
    track takes the nearest truth no earlier track of the scan has taken, if it lies within ``gate`` metres (strict).

    Returns a namespace: ``posRMSE`` [Q] and ``velRMSE`` [Q], the root mean square of the position and the velocity error of truth q over the scans in which a confirmed
    track was matched to it (NaN where there is none); ``nScans`` [Q], the number of those scans; ``idSwitches``, the number of times the id matched to a truth differs
    from the id matched to it the time before; ``falseTracks``, the number of distinct ids that were confirmed in some scan and matched in none; ``match`` [S x Q], the
    id matched to truth q in scan s, or 0."""
    truth = np.asarray(truth, dtype=np.float64)
    if truth.ndim != 3 or truth.shape[2] not in (2, 4) or truth.shape[0] != len(history):
        raise ValueError("getTrackRMSE: truth must be [scans x targets x 4] or [scans x targets x 2], one scan per history entry")
    S, Q, W = truth.shape
    match = np.zeros((S, Q), dtype=np.int64)
    pe2, ve2, cnt = np.zeros(Q), np.zeros(Q), np.zeros(Q, dtype=np.int64)
    confirmed, matched = set(), set()
    for s, scan in enumerate(history):
        tr = scan["tracks"][bank]
        free = np.ones(Q, dtype=bool)
        for i in np.flatnonzero(np.asarray(tr["status"]) == 2):
            tid, x = int(tr["id"][i]), np.asarray(tr["x"][i], dtype=np.float64)
            confirmed.add(tid)
            d = np.where(free, np.hypot(truth[s, :, 0] - x[0], truth[s, :, 1] - x[1]), np.inf)
            if d.size and np.isfinite(d).any():
                q = int(np.argmin(d))
                if d[q] < gate:
                    free[q] = False
                    match[s, q] = tid
                    matched.add(tid)
                    pe2[q] += d[q] ** 2
                    if W == 4:
                        ve2[q] += (truth[s, q, 2] - x[2]) ** 2 + (truth[s, q, 3] - x[3]) ** 2
                    cnt[q] += 1
    switches = 0
    for q in range(Q):
        ids = match[match[:, q] > 0, q]
        switches += int((ids[1:] != ids[:-1]).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        pos = np.where(cnt > 0, np.sqrt(pe2 / cnt), math.nan)
        vel = np.where(cnt > 0, np.sqrt(ve2 / cnt), math.nan) if W == 4 else np.full(Q, math.nan)
    return SimpleNamespace(posRMSE=pos, velRMSE=vel, nScans=cnt, idSwitches=switches, falseTracks=len(confirmed - matched), match=match)
