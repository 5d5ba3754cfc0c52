"""sensing.postProcessing.getRMSE (+sensing/+postProcessing/getRMSE.m:1-72)."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np


def _field(obj, name):
    return obj[name] if isinstance(obj, dict) else getattr(obj, name)


def _vec(x):
    return np.asarray(x, dtype=np.float64).reshape(-1)


def getRMSE(radarEstResults, radarEstParams):
    """radarEstRMSE = sensing.postProcessing.getRMSE(radarEstResults, radarEstParams): the error of every range estimate against the first true target within one range
    resolution cell of it, and of the velocity / azimuth (/ elevation, UPA only) estimates at the same index (getRMSE.m:42-61).

    ``radarEstResults``: the estResults of sensing.estimation.fft2D / music2D / redetect (``rngEst, velEst, aziEst, eleEst``), or the dict of
    sensing.estimation.targetList (``rng, vel, azi``) or, for a UPA, of sensing.estimation.targetListUPA (which adds ``ele``).  The reference indexes the three estimate lists with one index r although fft2D forms them independently
    (fft2D.m:96-99); the target list pairs them per detection, which makes it the meaningful input.  ``radarEstParams``: ``rRes``, ``antennaType`` and
    ``targetRealPos`` of sensing.radarParams -- the reference reads ``tgtRealPos``, a field radarParams.m never sets (radarParams.m:137-144 names it targetRealPos), and
    tests the array's MATLAB class; here the UPA test is ``antennaType.kind == "upa"``.

    For r < numel(rngEst): the first truth index with |rngReal - rngEst[r]| < rRes (strict, :43) gives real - est for range, velocity, azimuth and, for a UPA, elevation
    (:47-52); each output entry is sqrt(mean(rmmissing(err)^2)) of that single error (:56-59): |err|, or NaN when no truth matched.  Returns a namespace of
    ``rngRMSE, velRMSE, eleRMSE, aziRMSE`` [numel(rngEst)]; ``float('nan')`` when rngEst is empty (:31-35).  Raises ValueError when velEst, aziEst (or eleEst, UPA) is
    shorter than rngEst, where the reference's index runs past the end."""
    is_upa = getattr(_field(radarEstParams, "antennaType"), "kind", None) == "upa"                    # :13
    truth = _field(radarEstParams, "targetRealPos")
    rng_real, vel_real, ele_real, azi_real = (_vec([t[k] for t in truth]) for k in ("Range", "Velocity", "Elevation", "Azimuth"))   # :17-20
    if isinstance(radarEstResults, dict) and "rng" in radarEstResults:                                # sensing.estimation.targetList
        if is_upa and "ele" not in radarEstResults:                                                   # targetList's dict; targetListUPA's carries ele
            raise ValueError("getRMSE: the target list carries no elevation (it is refused for a UPA)")
        rng_est, vel_est, azi_est = _vec(radarEstResults["rng"]), _vec(radarEstResults["vel"]), _vec(radarEstResults["azi"])
        ele_est = _vec(radarEstResults["ele"]) if is_upa else None
    else:
        rng_est, vel_est, azi_est = (_vec(_field(radarEstResults, k)) for k in ("rngEst", "velEst", "aziEst"))   # :22-29
        ele_est = _vec(_field(radarEstResults, "eleEst")) if is_upa else None
    if rng_est.size == 0:                                                                             # :31-35
        return float("nan")
    n = rng_est.size                                                                                  # :38
    for name, v in (("velEst", vel_est), ("aziEst", azi_est), ("eleEst", ele_est)):
        if v is not None and v.size < n:
            raise ValueError(f"getRMSE: {name} has {v.size} entries, rngEst {n}")
    r_res = float(_field(radarEstParams, "rRes"))                                                     # :10
    out = SimpleNamespace(**{k: np.full(n, math.nan) for k in ("rngRMSE", "velRMSE", "eleRMSE", "aziRMSE")})   # :39-40
    for r in range(n):
        hit = np.flatnonzero(np.abs(rng_real - rng_est[r]) < r_res)                                   # :43
        if hit.size:                                                                                  # :45-53
            i = int(hit[0])
            out.rngRMSE[r] = abs(rng_real[i] - rng_est[r])                                            # :56-59: sqrt(mean(e^2)) of the one error
            out.velRMSE[r] = abs(vel_real[i] - vel_est[r])
            if is_upa:
                out.eleRMSE[r] = abs(ele_real[i] - ele_est[r])
            out.aziRMSE[r] = abs(azi_real[i] - azi_est[r])
    return out
