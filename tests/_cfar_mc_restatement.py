"""NumPy restatement of isac_cfar_monte_carlo (include/isac_cfar_mc.h; project-defined), the expressions its counts are compared with, and what its CPU
and GPU tests share.

Trial t, call j: Philox4x32-10 (oracle/philox.py), key (seed lo, seed hi), counter (t lo, t hi, 4, j); w0 = o0 | o1 << 32, w1 = o2 | o3 << 32; u(w) = ((w >> 11) + 1) 2^-53.
Training cells T_{2j+1} = -ln u(w0), T_{2j+2} = -ln u(w1), j = 0 .. N/2 - 1 (np.log).  CUT, call N/2: E0 = -ln u(w0), theta = 2 pi (w1 >> 11) 2^-53; with S = 10^(snr_db / 10):
Swerling 1 P = (1 + S) E0, Swerling 0 P = (sqrt(S) + sqrt(E0) cos theta)^2 + (sqrt(E0) sin theta)^2.  Detector: tests/_cfar_methods_restatement.py noise_estimate on
T_1 .. T_N (CA / GOCA / SOCA sums in order, OS by np.partition), thr = alpha * estimate, detection iff P > thr."""
from __future__ import annotations

import functools
import math

import numpy as np
from scipy import integrate, stats

from oracle.philox import philox4x32_10

import _cfar_methods_restatement as M

STREAM = 4                       # kCfarMcStream
MODELS = {"swerling0": 0, "swerling1": 1}
MARGIN = 1e-11                   # (trial, SNR point) pairs whose |P - thr| / max(P, thr) is not above this are left out of flag comparisons


def _words(t, j, seed):
    o = philox4x32_10((t & np.uint64(0xFFFFFFFF)).astype(np.uint32), (t >> np.uint64(32)).astype(np.uint32), np.uint32(STREAM), np.uint32(j),
                      np.uint32(seed & 0xFFFFFFFF), np.uint32((seed >> 32) & 0xFFFFFFFF))
    return o[0].astype(np.uint64) | (o[1].astype(np.uint64) << np.uint64(32)), o[2].astype(np.uint64) | (o[3].astype(np.uint64) << np.uint64(32))


def _neg_ln_u(w):
    return -np.log(((w >> np.uint64(11)).astype(np.float64) + 1.0) * 2.0 ** -53)


def draw(N, seed, n_trials, t0=0):
    """(T [N x n], E0 [n], theta [n]) of trials t0 .. t0 + n_trials - 1."""
    t = np.arange(t0, t0 + n_trials, dtype=np.uint64)
    T = np.empty((N, n_trials))
    for j in range(N // 2):
        w0, w1 = _words(t, j, seed)
        T[2 * j], T[2 * j + 1] = _neg_ln_u(w0), _neg_ln_u(w1)
    w0, w1 = _words(t, N // 2, seed)
    return T, _neg_ln_u(w0), 2.0 * np.pi * ((w1 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53)


@functools.lru_cache(maxsize=None)
def cached_draw(N, seed, n_trials):
    """draw(N, seed, n_trials), computed once and shared: read-only."""
    out = draw(N, seed, n_trials)
    for a in out:
        a.setflags(write=False)
    return out


def detect(drawn, method, rank, alpha, model, snr_db):
    """(flags [n x n_snr] uint8, margin [n x n_snr]) of the trials `drawn` = (T, E0, theta); margin = |P - thr| / max(P, thr)."""
    T, e0, theta = drawn
    thr = alpha * M.noise_estimate(T, method, rank)
    s = 10.0 ** (np.asarray(snr_db, dtype=np.float64) / 10.0)                  # -inf -> 0
    if MODELS[model] == 1:
        p = (1.0 + s)[None, :] * e0[:, None]
    else:
        r = np.sqrt(e0)
        p = (np.sqrt(s)[None, :] + (r * np.cos(theta))[:, None]) ** 2 + ((r * np.sin(theta)) ** 2)[:, None]
    flags = (p > thr[:, None]).astype(np.uint8)
    return np.asfortranarray(flags), np.abs(p - thr[:, None]) / np.maximum(p, thr[:, None])


# ---------------------------------------------------------------- the expressions the counts are compared with (exponential cells), written out here
def _soca(n, T):
    return 2.0 * math.fsum(math.comb(n - 1 + k, k) * (2.0 + T) ** -(n + k) for k in range(n))


def false_alarm(method, N, alpha, rank=1):
    n = N // 2
    if method == "CA":
        return (1.0 + alpha / N) ** -N
    if method == "SOCA":
        return _soca(n, alpha / n)
    if method == "GOCA":
        return 2.0 * (1.0 + alpha / n) ** -n - _soca(n, alpha / n)
    return math.prod((N - i) / (N - i + alpha) for i in range(rank))


def pd_swerling1(method, N, alpha, rank, snr_db):
    """An exponential target of mean S on unit noise is an exponential CUT of mean 1 + S: the false-alarm expression at alpha / (1 + S)."""
    return np.array([false_alarm(method, N, alpha / (1.0 + 10.0 ** (x / 10.0)), rank) for x in snr_db])


def pd_swerling0_ca(N, alpha, snr_db):
    """CA: the noise estimate is Z / N, Z ~ Gamma(N, 1); 2 P is noncentral chi-square with 2 degrees of freedom and noncentrality 2 S."""
    out = []
    for x in snr_db:
        s = 10.0 ** (x / 10.0)
        v, err = integrate.quad(lambda z: stats.gamma.pdf(z, N) * stats.ncx2.sf(2.0 * alpha * z / N, 2, 2.0 * s), 0.0, np.inf, epsabs=1e-13, epsrel=1e-11, limit=200)
        assert err < 1e-9
        out.append(v)
    return np.array(out)


def within_5_sigma(d, n, p):
    """|d - n p| <= 5 sqrt(n p (1 - p)); also returns the deviation in sigmas."""
    sigma = math.sqrt(n * p * (1.0 - p))
    return abs(d - n * p) <= 5.0 * sigma, (d - n * p) / sigma if sigma > 0 else 0.0
