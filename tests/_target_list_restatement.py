"""NumPy restatement of the per-target list of fft2D (include/isac_targets.h: isac_fft2d_get_targets, DESIGN.md section 5 -- project-defined), and the scenes its tests share.

Steps 1-5 on a power window P [nr x nc x A] (cell (0, 0) = rdm cell (first_row, first_col), 1-based), the per-antenna detection lists ([2 x D] arrays of 1-based rdm
coordinates, as the oracle's fft2d and isac_fft2d_get_detections give them), the CUT rectangle, and complex snapshots.  Besides the list it returns the two decision
margins of every target: margin 1 = how far S lies above its largest neighbour, margin 2 = how far the best Bartlett value lies above the best one that is not its
bitwise twin (same sind), both relative."""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np

import oracle as O
from oracle.music import ula_scan_angles

GUARD_BAND = 1e-9        # the project's own guard band ("no CUT within 1e-9 relative of threshold")


def integrated_map(P):
    """Step 1: S = sum_a P[:, :, a], fp64, ascending antenna order starting from 0.0."""
    S = np.zeros(P.shape[:2], dtype=np.float64)
    for a in range(P.shape[2]):
        S = S + P[:, :, a]
    return S


def hits_map(dets, shape, first_row, first_col):
    h = np.zeros(shape, dtype=np.int64)
    for d in dets:
        d = np.asarray(d).reshape(2, -1)
        np.add.at(h, (d[0] - first_row, d[1] - first_col), 1)
    return h


def target_cells(P, dets, first_row, first_col, rect, n_ifft):
    """Steps 1, 2 and 5 (the order): rows / cols (1-based rdm bins), hits, power, margin1, sorted by S descending, ties by ascending r + nIFFT (c - 1).
    ``near_miss``: the smallest relative distance by which a detected CUT cell that is NOT a target falls short of being one (inf when there is none)."""
    row0, row1, col0, col1 = rect
    if row0 - first_row < 1 or col0 - first_col < 1 or row1 - first_row + 1 >= P.shape[0] or col1 - first_col + 1 >= P.shape[1]:
        raise ValueError("the window carries no halo around the CUT zone")
    S = integrated_map(P)
    H = hits_map(dets, S.shape, first_row, first_col)
    rows, cols, hits, power, m1 = [], [], [], [], []
    near = math.inf
    for c in range(col0, col1 + 1):
        for r in range(row0, row1 + 1):
            i, j = r - first_row, c - first_col
            if H[i, j] < 1:
                continue
            nb = S[i - 1:i + 2, j - 1:j + 2].copy()
            v = nb[1, 1]
            nb[1, 1] = -np.inf
            big = nb.max() if not np.isnan(nb).any() else np.nan
            if v > big:                                    # strictly greater than all 8 neighbours; NaN compares false
                rows.append(r); cols.append(c); hits.append(int(H[i, j])); power.append(v); m1.append((v - big) / v)
            elif np.isfinite(v) and np.isfinite(big) and big > 0:
                near = min(near, (big - v) / big)
    rows, cols, hits = np.array(rows, dtype=np.int64), np.array(cols, dtype=np.int64), np.array(hits, dtype=np.int64)
    power, m1 = np.array(power, dtype=np.float64), np.array(m1, dtype=np.float64)
    order = np.lexsort((rows + n_ifft * (cols - 1), -power))
    return SimpleNamespace(row=rows[order], col=cols[order], hits=hits[order], power=power[order], margin1=m1[order], near_miss=near, S=S, H=H)


def bartlett(x, rp):
    """Step 4 on snapshots x [A] or [A x n]: (bin, azi, margin2, B) -- the first arg-max of B(i) = |sum_m conj(a_i[m]) x[m]|^2 over the ULA scan grid of music.m:76-96."""
    x = np.asarray(x, dtype=np.complex128)
    x = x.reshape(x.shape[0], -1)
    ang = ula_scan_angles(rp)
    sd = np.array([float(O.sind(a)) for a in ang])
    m = np.arange(x.shape[0], dtype=np.float64)
    arg = ((-2.0 * np.pi) * m)[None, :] * 0.5 * sd[:, None]            # left to right, as the device and music.m:82
    steer = np.exp(1j * arg)                                            # a_i[m]
    B = np.abs(np.conj(steer) @ x) ** 2                                 # [steps x n]
    bins = np.argmax(B, axis=0)
    margin2 = np.empty(x.shape[1])
    for t, b in enumerate(bins):
        other = B[sd != sd[b], t]
        margin2[t] = (B[b, t] - other.max()) / B[b, t]
    return bins, ang[bins].astype(np.float64), margin2, B


def target_list(P, dets, first_row, first_col, rect, rp, snapshot_of):
    """Steps 1-5.  ``snapshot_of(rows, cols)`` -> x [A x n] (step 3: rdm values at those 1-based cells, or a device's snapshots)."""
    t = target_cells(P, dets, first_row, first_col, rect, int(rp.nIFFT))
    x = snapshot_of(t.row, t.col) if t.row.size else np.zeros((P.shape[2], 0), dtype=np.complex128)
    t.snapshots = x
    if t.row.size:
        t.bin, t.azi, t.margin2, _ = bartlett(x, rp)
    else:
        t.bin, t.azi, t.margin2 = np.zeros(0, dtype=np.int64), np.zeros(0), np.zeros(0)
    t.rng = (t.row - 1) * rp.rRes                                        # fft2D.m:77,:81
    t.vel = (t.col - int(rp.nFFT) / 2 - 1) * rp.vRes                     # fft2D.m:78,:82
    return t


# ---------------------------------------------------------------- the scenes of tests/test_target_list_cpu.py (conditioning) and tests/test_gpu_target_list.py
# Two targets at ranges ~106 m and ~182 m with velocities of opposite sign.  fft2D.m:44 swaps the two halves of the symbol axis, so a target whose Doppler phase
# advances by a fraction of a turn over L symbols shows a SPLIT Doppler peak (two lobes 2 dB apart) that outranks the weaker target (-10 dB): the 273-PRB scenes put
# the targets at +-nFFT/L Doppler bins, where the swap leaves the tone continuous and only the -13 dB sidelobes of the unwindowed Doppler axis remain.  No zeroed 'S'
# slot, for the same reason: a gap in the slow-time sequence raises lobes 7 bins from the peak.
_POS = ((100.0, 20.0, 1.5), (178.0, -36.0, 1.5))
_V273 = 4.5621831158455395 * 256 / 56                                                         # vRes (SURVEY KAT-2) x nFFT / L
_TWO = dict(targets=_POS, velocity=(_V273, -_V273), zero_s_slots=False)
_TWO24 = dict(targets=_POS, velocity=(7.0, -9.0), zero_s_slots=False)
SCENES = {
    # K = 3276, nFFT = 256: doppler_fft256_kernel.  L = 56 (n_slots = 4), not 28: with 28 symbols zero-padded to 256 Doppler bins the main lobe is 18 bins wide, the
    # training cells 3 bins from the CUT sit inside it, and CA-CFAR (alpha = 32.9) detects nothing at all -- a scene without a target checks nothing
    "a4_273prb": dict(n_ants=4, n_slots=4, seed=21, **_TWO),
    "a8_273prb": dict(n_ants=8, n_slots=4, seed=22, **_TWO),
    "a4_24prb_generic": dict(n_ants=4, n_slots=2, nrb=24, num_slots_param=6, seed=23, **_TWO24),   # nIFFT = 512, nFFT = 64 > L: the generic Doppler kernel, zero-padded
    "a4_24prb_truncated": dict(n_ants=4, n_slots=2, nrb=24, num_slots_param=1, seed=24, **_TWO24),  # nFFT = 16 < L = 28: truncation
}

# The same two targets at CFAR bands other than the default GuardBandSize (2, 2), TrainingBandSize (1, 1): hr = 4 != hc = 5 (neither the default 3) and gr = 1 != gc = 3, so every reader of the CPI's
# window (the re-detection, this list, the refinement, the beam planes, the cancellation passes) sees a window whose row and column halves differ, a guard block that is not
# square and -- GOCA / SOCA -- a front / rear split of 78 training cells.  The three guard columns step over the Doppler main lobe, so the default Pfa still detects.
READER_BANDS = ((1, 3), (3, 2))
DEFAULT_BANDS = ((2, 2), (1, 1))                                                              # cfar2D.m:32-33
BAND_SCENE = "a4_273prb_g13_t32"
SCENES[BAND_SCENE] = dict(n_ants=4, n_slots=4, seed=26, **_TWO)
BANDS = {BAND_SCENE: READER_BANDS}                                                            # scene name -> (guard, train); every other scene: the default


def bands_of(name):
    return BANDS.get(name, DEFAULT_BANDS)


def oracle_config(name, rp):
    """O.cfar2d_config at the scene's bands."""
    cf = O.cfar2d_config(rp)
    cf.GuardBandSize, cf.TrainingBandSize = bands_of(name)
    return cf


def with_bands(name, cfar):
    """The library's cfarConfig with the scene's bands set on its detector (the user setting: cf.cfarDetector2D.GuardBandSize = ...)."""
    cfar.cfarDetector2D.GuardBandSize, cfar.cfarDetector2D.TrainingBandSize = bands_of(name)
    return cfar


# One target, 8 elements: only the conditioning test runs it (ORACLE_ONLY), to record that the Bartlett azimuth of the list is NOT fft2D's aziEst.
ORACLE_ONLY = {"a8_single": dict(n_ants=8, n_slots=4, seed=25, targets=(_POS[0],), velocity=(_V273,), zero_s_slots=False)}


def make(name):
    from conftest import make_scene
    return make_scene(**{**SCENES, **ORACLE_ONLY}[name])


@functools.lru_cache(maxsize=None)
def oracle_targets(name):
    """The oracle-only result: O.mono_static_sensing -> rdm -> the oracle CFAR -> the restatement.  Computed once per scene and shared; callers must not modify it."""
    sc = make(name)
    cf = oracle_config(name, sc.rp)
    echo = O.mono_static_sensing(sc.tx_wave, sc.tx_grid.shape, sc.carrier, sc.rp, sc.los, sc.noise, nfft=sc.wave.Nfft)
    est, dbg = O.fft2d(sc.rp, cf, echo, sc.tx_grid, return_debug=True, rdm_fn=O.rdm_explicit)
    rect = (cf.rowRange[0], cf.rowRange[1], cf.colRange[0], cf.colRange[1])
    hr, hc = cf.GuardBandSize[0] + cf.TrainingBandSize[0], cf.GuardBandSize[1] + cf.TrainingBandSize[1]
    fr, fc = rect[0] - hr, rect[2] - hc
    win = dbg.rdm[fr - 1:rect[1] + hr, fc - 1:rect[3] + hc, :].copy()      # the complex window; the full map is not kept
    t = target_list(np.abs(win) ** 2, dbg.detections, fr, fc, rect, sc.rp, lambda r, c: win[r - fr, c - fc, :].T)
    t.rdm_max = float(np.abs(dbg.rdm).max())
    t.rdm_at = lambda r, c: win[np.asarray(r) - fr, np.asarray(c) - fc, :].T
    t.est, t.rect, t.first_row, t.first_col = est, rect, fr, fc
    return t
