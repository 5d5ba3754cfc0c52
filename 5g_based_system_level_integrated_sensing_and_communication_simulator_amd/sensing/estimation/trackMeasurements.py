"""sensing.estimation.trackMeasurements: a localizeTargets result and / or a linkMeasurements record -> the measurement record of sensing.estimation.Tracker (host helper;
project-defined, include/isac_track.h)."""
from __future__ import annotations

import numpy as np


def trackMeasurements(fixes=None, sigmaPos=None, sigmaVel=None, links=None):
    """One scan's record ``group, kind, link, z [M x 4], sigma [M x 4]`` for one bank.

    ``fixes``: the dict of sensing.estimation.localizeTargets (``pos`` [n x 2], ``vel`` [n x 2], ``vel_status`` [n]) -> kind-0 measurements (x, y, vx, vy) in group 0 with
    the standard deviations ``sigmaPos`` (metres) and ``sigmaVel`` (m/s); vx and vy are NaN (absent) where ``vel_status`` is 1.  ``links``: the record of
    sensing.estimation.linkMeasurements -> kind-1 measurements (r, azi, s) with its sigmas, link k in group 1 + k (so K <= 255).  Either source may be absent.  A sigma
    nothing reads (the fourth of a link measurement, those of absent components) is 1."""
    group, kind, link, z, sigma = [], [], [], [], []
    if fixes is not None:
        if sigmaPos is None or sigmaVel is None:
            raise ValueError("trackMeasurements: fixes need sigmaPos and sigmaVel")
        pos = np.asarray(fixes["pos"], dtype=np.float64).reshape(-1, 2)
        n = pos.shape[0]
        vel = np.asarray(fixes["vel"], dtype=np.float64).reshape(-1, 2) if "vel" in fixes else np.full((n, 2), np.nan)
        if vel.shape[0] != n:
            raise ValueError("trackMeasurements: pos and vel differ in length")
        if "vel_status" in fixes:
            vel = np.where((np.asarray(fixes["vel_status"]).reshape(-1) == 1)[:, None], np.nan, vel)
        group.append(np.zeros(n, dtype=np.int32)); kind.append(np.zeros(n, dtype=np.int32)); link.append(np.zeros(n, dtype=np.int32))
        z.append(np.hstack([pos, vel]))
        sigma.append(np.tile([float(sigmaPos), float(sigmaPos), float(sigmaVel), float(sigmaVel)], (n, 1)))
    if links is not None:
        lk = np.asarray(links["link"], dtype=np.int32).reshape(-1)
        n = lk.size
        f = {k: np.asarray(links[k], dtype=np.float64).reshape(-1) for k in ("r", "azi", "s", "sigma_r", "sigma_a", "sigma_v")}
        if any(a.size != n for a in f.values()):
            raise ValueError("trackMeasurements: the link record's fields differ in length")
        if n and int(lk.max()) > 254:
            raise ValueError("trackMeasurements: link k goes to group 1 + k, so k <= 254")
        group.append(1 + lk); kind.append(np.ones(n, dtype=np.int32)); link.append(lk)
        z.append(np.column_stack([f["r"], f["azi"], f["s"], np.zeros(n)]))
        sigma.append(np.column_stack([f["sigma_r"], f["sigma_a"], f["sigma_v"], np.ones(n)]))
    cat = lambda parts, shape, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(shape, dtype=dt)   # noqa: E731
    return dict(group=cat(group, 0, np.int32), kind=cat(kind, 0, np.int32), link=cat(link, 0, np.int32), z=cat(z, (0, 4), np.float64), sigma=cat(sigma, (0, 4), np.float64))
