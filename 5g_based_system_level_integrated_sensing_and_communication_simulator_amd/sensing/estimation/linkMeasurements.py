"""sensing.estimation.linkMeasurements: per-link target lists -> the measurement record of sensing.estimation.localizeTargets (host helper; project-defined)."""
from __future__ import annotations

import numpy as np


def linkMeasurements(lists, links, radarParams, sigmaRange=None, sigmaVel=None, sigmaAzi=2.0, useAzimuth=True):
    """One list per link -> ``link, r, s, azi, sigma_r, sigma_v, sigma_a`` [M].

    ``lists[k]``: the list of link ``links[k]`` = (tx node, rx node), formed by the rx node with the tx node's transmit grid -- the dict of sensing.estimation.targetList,
    refineTargets, refineRange, cleanTargets or relaxTargets: anything with ``rng``, ``vel`` and ``azi``.  A list's range axis is half the path length and its velocity
    axis half the Doppler sum (a mono-static list reads them as range and radial speed), so r = 2 rng and s = 2 vel; ``azi`` is already the azimuth seen from the rx
    node.  Entries flagged ``sidelobe_of`` >= 0 (refineTargets) are dropped.  ``sigmaRange`` (default rRes), ``sigmaVel`` (default vRes) and ``sigmaAzi`` (degrees) are
    the standard deviations given to every measurement; ``useAzimuth=False`` sets every azimuth to NaN (not used).  ``index`` [M] is the entry's position in its list."""
    if len(lists) != len(np.asarray(links).reshape(-1, 2)):
        raise ValueError("linkMeasurements: one list per link")
    s_r = float(radarParams.rRes if sigmaRange is None else sigmaRange)
    s_v = float(radarParams.vRes if sigmaVel is None else sigmaVel)
    link, index, r, s, azi = [], [], [], [], []
    for k, tl in enumerate(lists):
        rng, vel, az = (np.asarray(tl[f], dtype=np.float64).reshape(-1) for f in ("rng", "vel", "azi"))
        if not rng.size == vel.size == az.size:
            raise ValueError(f"linkMeasurements: list {k}: rng, vel and azi differ in length")
        keep = np.ones(rng.size, dtype=bool) if "sidelobe_of" not in tl else np.asarray(tl["sidelobe_of"]).reshape(-1) < 0
        for i in np.flatnonzero(keep):
            link.append(k); index.append(int(i)); r.append(2.0 * rng[i]); s.append(2.0 * vel[i]); azi.append(az[i] if useAzimuth else np.nan)
    n = len(link)
    return dict(link=np.asarray(link, dtype=np.int32), index=np.asarray(index, dtype=np.int32), r=np.asarray(r, dtype=np.float64), s=np.asarray(s, dtype=np.float64),
                azi=np.asarray(azi, dtype=np.float64), sigma_r=np.full(n, s_r), sigma_v=np.full(n, s_v), sigma_a=np.full(n, float(sigmaAzi)))
