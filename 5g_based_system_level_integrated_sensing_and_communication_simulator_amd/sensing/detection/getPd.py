"""sensing.detection.getPd (+sensing/+detection/getPd.m:1-12), without the plot (getPd.m:14-20)."""
from __future__ import annotations

import math

import numpy as np


def _erfcinv(y: float) -> float:
    """x with erfc(x) = y, 0 < y < 2.  Newton on ln erfc(x) - ln y, which is concave and falling: after the first step the iterates come down on the root from the
    right, nearly quadratically (ln erfc ~ -x^2).  Accurate to the rounding of math.erfc."""
    if not 0.0 < y < 2.0:
        raise ValueError("erfcinv: argument outside (0, 2)")
    if y > 1.0:
        return -_erfcinv(2.0 - y)
    x, ln_y = 0.0, math.log(y)
    for _ in range(100):
        e = math.erfc(x)
        step = (math.log(e) - ln_y) * e / (2.0 / math.sqrt(math.pi) * math.exp(-x * x))
        if x + step == x:
            break
        x += step
    return x


def getPd(Pfa, snrdB, nPulses):
    """Pd = sensing.detection.getPd(Pfa, snrdB, nPulses): the receiver operating characteristic rocpfa(Pfa, 'MaxSNR', snrdB(end), 'MinSNR', snrdB(1), 'NumPoints',
    numel(snrdB), 'NumPulses', nPulses) returns (getPd.m:9-12).  ``Pd`` [numel(snrdB) x numel(Pfa)], evaluated -- as the reference passes only Min, Max and NumPoints --
    at linspace(snrdB[0], snrdB[-1], numel(snrdB)) dB, whatever lies between the ends of ``snrdB``.

    rocpfa's default signal type, 'NonfluctuatingCoherent', as the toolbox documents it:  Pd = 1/2 erfc(erfcinv(2 Pfa) - sqrt(nPulses snr)).  The toolbox itself is not
    available to this project, so the formula is taken from its documentation and has not been compared with rocpfa's output.  It describes a FIXED
    threshold receiver: the detection rate of the CFAR detectors this library runs, CFAR loss included, is what sensing.detection.cfarMonteCarlo measures.  Host only."""
    pfa = np.atleast_1d(np.asarray(Pfa, dtype=np.float64)).reshape(-1)
    snr_db = np.atleast_1d(np.asarray(snrdB, dtype=np.float64)).reshape(-1)
    if snr_db.size == 0 or pfa.size == 0:
        return np.zeros((snr_db.size, pfa.size))
    if not ((pfa > 0.0) & (pfa < 1.0)).all():
        raise ValueError("Pfa must lie in (0, 1)")
    snr = 10.0 ** (np.linspace(snr_db[0], snr_db[-1], snr_db.size) / 10.0)
    root = np.sqrt(float(nPulses) * snr)
    pd = np.empty((snr.size, pfa.size))
    for k, p in enumerate(pfa):
        x = _erfcinv(2.0 * float(p))
        pd[:, k] = [0.5 * math.erfc(x - r) for r in root]
    return pd
