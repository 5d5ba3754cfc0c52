"""sensing.detection.cfarMonteCarlo: the false-alarm and detection rates of the library's CFAR detectors by counting on the GPU (project-defined; include/isac_cfar_mc.h,
isac_cfar_monte_carlo)."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np

from ... import _lib as L
from .cfarDetect import cfarThresholdFactor, method_block


def cfarMonteCarlo(nTrain_or_cfarConfig, snrdB, nTrials, *, Method="CA", Rank=1, ThresholdFactor="Auto", CustomThresholdFactor=None, Pfa=None, model="swerling0", seed=0,
                   return_flags=False, ctx=None):
    """Draw ``nTrials`` noise windows of N unit-mean exponential training cells, a CUT holding noise plus a target at each SNR of ``snrdB`` (dB; ``-inf`` is the
    false-alarm point), run the detector ``Method`` / ``Rank`` / ``ThresholdFactor`` on each and count.

    ``nTrain_or_cfarConfig``: N itself (even, 2..128; then ``Pfa`` is needed for ThresholdFactor 'Auto'), or the cfarConfig of sensing.detection.cfar2D, whose guard and
    training bands give N and whose ProbabilityFalseAlarm is used unless ``Pfa`` overrides it.  ``model``: 'swerling0' (non-fluctuating) or 'swerling1' (exponential target
    power).  Every SNR point of a trial sees the same noise, and trial t depends on (``seed``, t) alone: a shorter run is a prefix of a longer one.

    Returns a namespace: ``Pd`` [numel(snrdB)] = nDet / nTrials, ``nDet`` (uint64), ``nTrials``, ``alpha`` (the factor used), ``stderr`` = sqrt(Pd (1 - Pd) / nTrials), and
    with ``return_flags`` (nTrials <= 2^22) ``flags`` [nTrials x numel(snrdB)] uint8."""
    det = getattr(nTrain_or_cfarConfig, "cfarDetector2D", None)
    if det is not None:
        (g0, g1), (t0, t1) = det.GuardBandSize, det.TrainingBandSize
        n = (2 * (g0 + t0) + 1) * (2 * (g1 + t1) + 1) - (2 * g0 + 1) * (2 * g1 + 1)
        Pfa = det.ProbabilityFalseAlarm if Pfa is None else Pfa
    else:
        n = int(nTrain_or_cfarConfig)
    if model not in L.TARGET_MODELS:
        raise ValueError(f"model must be one of {list(L.TARGET_MODELS)}")
    m = method_block(Method, Rank, ThresholdFactor, CustomThresholdFactor)
    if ThresholdFactor == "Auto" and Pfa is None:
        raise ValueError("ThresholdFactor 'Auto' needs Pfa (or a cfarConfig that carries it)")
    pfa = 0.5 if Pfa is None else float(Pfa)                             # 'Custom': not used
    snr = L.as_f64(snrdB)
    n_trials = int(nTrials)
    ctx = ctx or L.default_context()
    n_det = np.zeros(max(snr.size, 1), dtype=np.uint64)
    flags = np.zeros((n_trials, snr.size), dtype=np.uint8, order="F") if return_flags and 0 < n_trials <= (1 << 22) else None
    if return_flags and flags is None:
        raise ValueError("return_flags needs 1 <= nTrials <= 2^22")
    ctx.check(ctx.lib.isac_cfar_monte_carlo(ctx.handle, C.byref(m), n, pfa, L.TARGET_MODELS[model], snr.ctypes.data_as(C.c_void_p), snr.size, n_trials,
                                            int(seed) & 0xFFFFFFFFFFFFFFFF, n_det.ctypes.data_as(C.c_void_p), None if flags is None else flags.ctypes.data_as(C.c_void_p)))
    n_det = n_det[: snr.size]
    pd = n_det.astype(np.float64) / n_trials
    out = SimpleNamespace(Pd=pd, nDet=n_det, nTrials=n_trials, stderr=np.sqrt(pd * (1.0 - pd) / n_trials),
                          alpha=m.custom_factor if ThresholdFactor == "Custom" else cfarThresholdFactor(Method, n, pfa, Rank=Rank))
    if return_flags:
        out.flags = flags
    return out
