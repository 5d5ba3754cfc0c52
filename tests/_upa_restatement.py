"""NumPy restatement of the reference's UPA DoA branch (music.m:31-71, digitalBF.m:13-53, mvdrBF.m:13-53) and of the project's
find2DPeaks (include/isac.h, isac_find2d_peaks) -- test infrastructure for tests/test_upa_doa_cpu.py and tests/test_gpu_upa_doa.py.

The reference evaluates the spectrum one scan point at a time (music.m:50-58): identical steering vectors give identical values.  A
vectorised product does not promise that (BLAS kernels may round two equal columns differently), so the quadratic forms below are
evaluated once per DISTINCT steering vector and scattered back; abs and mag2db likewise once per distinct value.  The mirror twins
(ph -+ 180, -th) then tie exactly here as they do in the reference and on the device.
"""
from __future__ import annotations

import math

import numpy as np
from scipy import linalg

from oracle.matlab_compat import EPS, cosd, mag2db, sind
from oracle.music import _noise_projector, determine_num_targets

D = 0.5   # music.m:12


def grid(rp):
    """music.m:36-53: elevation rows (eSteps) and azimuth columns (aSteps) in degrees."""
    a_gran, e_gran = float(rp.azimuthScanGranularity), float(rp.elevationScanGranularity)
    a_max, e_max = float(rp.azimuthScanScale), float(rp.elevationScanScale)
    a_steps = int(math.floor((a_max + 1) / a_gran))                       # :42
    e_steps = int(math.floor((e_max + 1) / e_gran))                       # :43
    return np.arange(e_steps) * e_gran - e_max / 2.0, np.arange(a_steps) * a_gran - a_max / 2.0   # :51-52


def steering_phases(n_v, n_h, ele, azi):
    """Phase of aUPA(ph, th, m, n) = exp(-2j pi sind(th) (m d cosd(ph) + n d sind(ph))) (music.m:44-55) for every grid point, column-major
    (e fastest), elements r = n + nH m (reshape of the [nH x nV] matrix, :54): [eSteps aSteps x nV nH]."""
    m = np.repeat(np.arange(n_v, dtype=np.float64), n_h)                 # r = n + nH m
    n = np.tile(np.arange(n_h, dtype=np.float64), n_v)
    ee, aa = np.meshgrid(np.arange(ele.size), np.arange(azi.size), indexing="ij")
    ee, aa = ee.ravel(order="F"), aa.ravel(order="F")
    sth, cph, sph = sind(ele)[ee], cosd(azi)[aa], sind(azi)[aa]
    inner = (m[None, :] * D) * cph[:, None] + (n[None, :] * D) * sph[:, None]
    return ((-2.0 * np.pi) * sth)[:, None] * inner + 0.0                  # (+ 0.0: one zero, so that equal phases compare equal as bytes)


_CACHE = {}


def unique_steering(n_v, n_h, rp):
    """(distinct steering vectors [A x U], inverse index [eSteps aSteps], eSteps, aSteps), cached per array and grid."""
    ele, azi = grid(rp)
    key = (n_v, n_h, ele.size, azi.size, float(ele[0]), float(azi[0]))
    if key not in _CACHE:
        ph = steering_phases(n_v, n_h, ele, azi)
        _, first, inv = np.unique(np.ascontiguousarray(ph).view(np.dtype((np.void, ph.shape[1] * 8))).ravel(), return_index=True, return_inverse=True)
        _CACHE[key] = (np.exp(1j * ph[first]).T.copy(), inv.ravel(), ele.size, azi.size)
    return _CACHE[key]


def _per_value(fn, x):
    u, inv = np.unique(x, return_inverse=True)
    return fn(u)[inv.ravel()].reshape(x.shape)


def spectrum_db(method, ra, n_v, n_h, rp, num_dets=None):
    """PdB [eSteps x aSteps] and L of music (method 0) / digitalBF (1) / mvdrBF (2) on Ra."""
    ra = np.asarray(ra, dtype=np.complex128)
    L = None
    if method == 0:
        L = determine_num_targets(np.real(linalg.eigvalsh(ra))) if num_dets is None else int(num_dets)   # music.m:21-24
        op, _ = _noise_projector(ra, L)                                    # :19-29  Uann
    elif method == 1:
        op = ra                                                            # digitalBF.m:38
    else:
        op = np.linalg.inv(ra)                                             # mvdrBF.m:38
    sv, inv, e_steps, a_steps = unique_steering(n_v, n_h, rp)
    q = np.einsum("rj,rj->j", sv.conj(), op @ sv)                        # aa' * M * aa per distinct vector
    p = q if method == 1 else 1.0 / (q + EPS)                              # music.m:56, mvdrBF.m:38
    absp = _per_value(np.abs, p)                                          # (complex abs per distinct value)
    pm = -absp[inv].reshape((e_steps, a_steps), order="F")                # :61  P = -abs(P)
    pnorm = pm / pm.max(axis=0)[None, :]                                  # :62  COLUMN-wise max
    with np.errstate(divide="ignore"):
        return _per_value(mag2db, pnorm), L                               # :63


def find_2d_peaks(pdb, n_peaks):
    """The project's find2DPeaks: interior cells strictly above all 8 neighbours, stable descending sort of find(isPeak) (column-major),
    the first min(L, #); returns 1-based (ele, azi)."""
    pdb = np.asarray(pdb, dtype=np.float64)
    if n_peaks <= 0:
        raise ValueError("find2DPeaks needs a positive number of peaks")
    rows, cols = pdb.shape
    is_peak = np.zeros_like(pdb, dtype=bool)
    if rows >= 3 and cols >= 3:
        c = pdb[1:-1, 1:-1]
        ok = np.ones_like(c, dtype=bool)
        for de in (-1, 0, 1):
            for da in (-1, 0, 1):
                if de or da:
                    ok &= c > pdb[1 + de:rows - 1 + de, 1 + da:cols - 1 + da]
        is_peak[1:-1, 1:-1] = ok
    lin = np.flatnonzero(is_peak.ravel(order="F"))                        # find(isPeak): column-major
    vals = pdb.ravel(order="F")[lin]
    order = np.argsort(-vals, kind="stable")[: int(n_peaks)]
    lin = lin[order]
    return lin % rows + 1, lin // rows + 1


def doa(method, ra, n_v, n_h, rp, num_dets=None):
    """(L, aziEst, eleEst, PdB) of the UPA branch (music.m:65-71)."""
    pdb, L = spectrum_db(method, ra, n_v, n_h, rp, num_dets)
    n = L if method == 0 else int(num_dets)
    ele, azi = find_2d_peaks(pdb, n)
    ele_est = (ele - 1) * rp.elevationScanGranularity - rp.elevationScanScale / 2.0   # :70
    azi_est = (azi - 1) * rp.azimuthScanGranularity - rp.azimuthScanScale / 2.0       # :71
    return L, azi_est.astype(np.float64), ele_est.astype(np.float64), pdb


def twin_columns(a_steps, a_gran=1.0, a_max=360.0):
    """Column of the azimuth ph -+ 180 for every column (the default 361-point grid)."""
    half = int(round(180.0 / a_gran))
    a = np.arange(a_steps)
    return np.where(a < half, a + half, a - half)
