"""NumPy restatement of step 4 of the UPA per-target list (include/isac_targets_upa.h: isac_fft2d_get_targets_upa, DESIGN.md section 5 -- project-defined), the scenes its
tests share and their oracle-only result.  Steps 1, 2, 3 and 5 are those of the ULA list: tests/_target_list_restatement.py.

Step 4: B(j) = |sum_r conj(a_j[r]) x[r]|^2 over the eSteps x aSteps grid of music.m:36-53, j = e + eSteps a, first arg-max.  B is evaluated once per DISTINCT steering
vector (tests/_upa_restatement.py: unique_steering) and scattered back, so the mirror twins (-th, ph -+ 180) tie exactly here as they do on the device, and the first
arg-max in column-major order is the lower twin.  margin 2 = how far the best value lies above the best value of a DIFFERENT steering vector, relative.

oracle.fft2d raises NotImplementedError for a UPA (music.m:69), so the oracle-only result is built from the stage functions: O.mono_static_sensing -> O.rdm_explicit ->
oracle.fft2d.detect_per_antenna -> the restatement."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import oracle as O
from oracle.fft2d import detect_per_antenna

import _target_list_restatement as T
import _upa_restatement as U

GUARD_BAND = T.GUARD_BAND


def bartlett2d(x, n_v, n_h, rp):
    """Step 4 on snapshots x [A] or [A x n]: (j, azi, ele, margin2, ties) -- j = e + eSteps a of the first arg-max, the angles in degrees (music.m:70-71), margin 2 and the
    number of grid points that carry the winning steering vector."""
    x = np.asarray(x, dtype=np.complex128)
    x = x.reshape(x.shape[0], -1)
    sv, inv, e_steps, a_steps = U.unique_steering(n_v, n_h, rp)
    ele_g, azi_g = U.grid(rp)
    n = x.shape[1]
    js, margin2, ties = np.zeros(n, dtype=np.int64), np.zeros(n), np.zeros(n, dtype=np.int64)
    for t in range(n):
        b = np.abs(sv.conj().T @ x[:, t]) ** 2                  # one value per distinct steering vector
        j = int(np.argmax(b[inv]))                              # first arg-max in column-major order
        u = int(inv[j])
        other = np.delete(b, u)
        margin2[t] = (b[u] - other.max()) / b[u] if other.size else 1.0
        js[t], ties[t] = j, int((inv == u).sum())
    return js, azi_g[js // e_steps].astype(np.float64), ele_g[js % e_steps].astype(np.float64), margin2, ties


def lowest_equal(j, n_v, n_h, rp):
    """The lowest grid index whose steering vector is bitwise the one of j (j itself, or its mirror twin)."""
    _, inv, _, _ = U.unique_steering(n_v, n_h, rp)
    return int(np.flatnonzero(inv == inv[int(j)])[0])


def bartlett2d_brute(x, n_v, n_h, rp):
    """Step 4 without `unique`: one grid point at a time, the same function on every point's own phase row (equal rows give equal values); the first arg-max.
    For coarse grids only."""
    ele_g, azi_g = U.grid(rp)
    ph = U.steering_phases(n_v, n_h, ele_g, azi_g)
    best, best_j = -1.0, -1
    for j in range(ph.shape[0]):
        b = abs(np.vdot(np.exp(1j * ph[j]), x)) ** 2            # |sum_r conj(a_j[r]) x[r]|^2
        if b > best:
            best, best_j = b, j
    return best_j


# ---------------------------------------------------------------- the scenes of tests/test_target_list_upa_cpu.py (conditioning) and tests/test_gpu_target_list_upa.py
# The smallest shapes at which each code path can go wrong: 2 x 4 against 4 x 2 catches a swapped m / n; 24 PRB (nIFFT 512) with nFFT 64 > L = 28 (zero-padded Doppler) and
# nFFT 16 < L (truncation); 273 PRB with nFFT 256 (doppler_fft256_kernel); and one scene per steering-tile width the 2-D scan dispatches on (A <= 64 / 128 / 256).
_POS = ((100.0, 20.0, 1.5), (178.0, -36.0, 1.5))
_V273 = 4.5621831158455395 * 256 / 56                                                         # vRes (SURVEY KAT-2) x nFFT / L
_S24 = dict(n_slots=2, nrb=24, num_slots_param=6, targets=_POS, velocity=(7.0, -9.0), zero_s_slots=False)
SCENES = {
    "upa2x2_24prb": dict(nV=2, nH=2, seed=41, **_S24),
    "upa2x4_24prb": dict(nV=2, nH=4, seed=42, **_S24),
    "upa4x2_24prb_trunc": dict(nV=4, nH=2, seed=43, **{**_S24, "num_slots_param": 1}),
    "upa4x4_273prb": dict(nV=4, nH=4, seed=44, n_slots=4, targets=_POS, velocity=(_V273, -_V273), zero_s_slots=False),
    "upa8x8_24prb": dict(nV=8, nH=8, seed=45, **_S24),
    "upa8x16_24prb": dict(nV=8, nH=16, seed=46, **_S24),
    "upa16x16_24prb": dict(nV=16, nH=16, seed=47, **_S24),
}
# ... and the 273-PRB scene at the asymmetric bands every reader of the CPI's window is run at (tests/_target_list_restatement.py: READER_BANDS)
BAND_SCENE = "upa4x4_273prb_g13_t32"
SCENES[BAND_SCENE] = dict(nV=4, nH=4, seed=48, n_slots=4, targets=_POS, velocity=(_V273, -_V273), zero_s_slots=False)
T.BANDS[BAND_SCENE] = T.READER_BANDS


def make(name):
    """The scene with a planar array: sc.rp is the oracle's radarParams for it (make_scene's own was made for a ULA)."""
    from conftest import make_scene
    kw = dict(SCENES[name])
    n_v, n_h = kw.pop("nV"), kw.pop("nH")
    sc = make_scene(n_ants=n_v * n_h, **kw)
    sc.cell.gNBSenAntenna = SimpleNamespace(kind="upa", nV=n_v, nH=n_h, dV=0.5, dH=0.5)
    sc.rp = O.radar_params(sc.cell, sc.carrier, sc.wave)
    sc.nV, sc.nH = n_v, n_h
    return sc


@functools.lru_cache(maxsize=None)
def oracle_targets(name):
    """The oracle-only result, from the stage functions.  Computed once per scene and shared; callers must not modify it."""
    sc = make(name)
    rp = sc.rp
    cf = T.oracle_config(name, rp)
    echo = O.mono_static_sensing(sc.tx_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, sc.noise, nfft=sc.wave.Nfft)
    rdm = O.rdm_explicit(echo, sc.tx_grid, int(rp.nIFFT), int(rp.nFFT))
    dets, _, _ = detect_per_antenna(rdm, cf, rp.rRes, rp.vRes, int(rp.nFFT))
    rect = (cf.rowRange[0], cf.rowRange[1], cf.colRange[0], cf.colRange[1])
    hr, hc = cf.GuardBandSize[0] + cf.TrainingBandSize[0], cf.GuardBandSize[1] + cf.TrainingBandSize[1]
    fr, fc = rect[0] - hr, rect[2] - hc
    win = rdm[fr - 1:rect[1] + hr, fc - 1:rect[3] + hc, :].copy()          # the complex window; the full map is not kept
    t = T.target_cells(np.abs(win) ** 2, dets, fr, fc, rect, int(rp.nIFFT))
    t.rdm_at = lambda r, c: win[np.asarray(r) - fr, np.asarray(c) - fc, :].T
    t.snapshots = t.rdm_at(t.row, t.col) if t.row.size else np.zeros((sc.A, 0), dtype=np.complex128)
    t.j, t.azi, t.ele, t.margin2, t.ties = bartlett2d(t.snapshots, sc.nV, sc.nH, rp)
    t.rng = (t.row - 1) * rp.rRes                                           # fft2D.m:77,:81
    t.vel = (t.col - int(rp.nFFT) / 2 - 1) * rp.vRes                        # fft2D.m:78,:82
    t.rdm_max = float(np.abs(rdm).max())
    t.rect, t.first_row, t.first_col = rect, fr, fc
    return t
