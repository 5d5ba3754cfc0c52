"""sensing.estimation.beamWeights: matched weights for sensing.estimation.beamDetect (project-defined; include/isac_beams.h)."""
from __future__ import annotations

import numpy as np

from ..radarParams import LIGHTSPEED, steeringVector


def beamWeights(radarParams, azimuth, elevation=None):
    """W [A x B]: for each direction (``azimuth[b]``, ``elevation[b]``; degrees, elevation 0 when omitted and unused by a ULA) the element-wise SQUARE of the steering
    vector sensing.radarParams forms for it (radarParams.m:81-118, ULA and UPA, the same lambda quirk).  The square is the matched weight of the range-Doppler cell of a
    mono-static echo: transmit element a feeds receive element a, so the cell carries the two-way phase."""
    azi = np.atleast_1d(np.asarray(azimuth, dtype=np.float64))
    ele = np.zeros_like(azi) if elevation is None else np.atleast_1d(np.asarray(elevation, dtype=np.float64))
    if ele.shape != azi.shape or azi.ndim != 1:
        raise ValueError("azimuth and elevation must be vectors of the same length")
    rp = radarParams
    n = int(rp.nTxAnts)
    lam = LIGHTSPEED / float(rp.fc)
    cols = [steeringVector(rp.antennaType, n, lam, azi[b], ele[b]) for b in range(azi.size)]
    s = np.stack(cols, axis=1) if cols else np.zeros((n, 0), dtype=np.complex128)
    return np.asfortranarray(s * s)
