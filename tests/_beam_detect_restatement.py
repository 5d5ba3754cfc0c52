"""NumPy restatement of beamformed detection (include/isac_beams.h: isac_fft2d_beam_detect, DESIGN.md section 5 -- project-defined), the scenes and beam sets its tests
share, and their oracle-only result.

Steps 2-4 on a complex window Y [nr x nc x A] (cell (0, 0) = rdm cell (first_row, first_col), 1-based), weights W [A x B], the CUT rectangle, guard / training bands and a
detector.  Detection goes through tests/_cfar_methods_restatement.detect with alpha from its threshold_factor.  Every decision returns its margin:
  detection       |P / thr - 1| of every CUT of every beam (``margin_det``: the smallest one; ``det_ratio``: P / thr of every detection)
  local maximum   how far M lies above its largest neighbour, relative (``margin_max`` per target; ``near_miss``: the smallest relative shortfall of a detected CUT cell
                  that is NOT a target)
  b*              how far M lies above the largest beam value that is not bitwise M, relative (``margin_beam`` per target; 1.0 where every beam has the same value)
The oracle-only result is built from stage calls: O.mono_static_sensing -> O.rdm_explicit -> the window -> this restatement."""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np

import oracle as O
from oracle.fft2d import detect_per_antenna

import _cfar_methods_restatement as C
import _target_list_restatement as T
import _target_list_upa_restatement as U

GUARD_BAND = T.GUARD_BAND


# ---------------------------------------------------------------- step 2
def beam_norms(W):
    """n_b = sum_a |W[a, b]|^2, fp64, ascending a from 0.0."""
    n = np.zeros(W.shape[1], dtype=np.float64)
    for a in range(W.shape[0]):
        n = n + (W[a].real * W[a].real + W[a].imag * W[a].imag)
    return n


def beam_planes(Y, W):
    """Pb [nr x nc x B] = |sum_a conj(W[a, b]) Y[:, :, a]|^2 / n_b, the sum in ascending a from 0 (the device fuses each multiply-add; NumPy rounds twice)."""
    Y, W = np.asarray(Y, dtype=np.complex128), np.asarray(W, dtype=np.complex128)
    n = beam_norms(W)
    P = np.empty(Y.shape[:2] + (W.shape[1],), dtype=np.float64, order="F")
    for b in range(W.shape[1]):
        z = np.zeros(Y.shape[:2], dtype=np.complex128)
        for a in range(Y.shape[2]):
            z = z + np.conj(W[a, b]) * Y[:, :, a]
        P[:, :, b] = (z.real * z.real + z.imag * z.imag) / n[b]
    return P


# ---------------------------------------------------------------- step 3
def detect_planes(P, first_row, first_col, rect, guard, train, method, alpha, rank=1):
    """Per-plane lists in CUT order, in rdm coordinates ([2 x D], 1-based), the CUTs' powers, P / thr of every detection and the smallest |P / thr - 1| over every CUT."""
    cuts = C.rectangle_cuts(rect)
    local = cuts - np.array([[first_row - 1], [first_col - 1]])
    dets, pows, ratios, margin = [], [], [], math.inf
    for b in range(P.shape[2]):
        d, thr = C.detect(P[:, :, b], local, guard, train, method, alpha, rank, return_threshold=True)
        p_cut = P[local[0] - 1, local[1] - 1, b]
        hit = p_cut > thr
        ok = np.isfinite(thr) & (thr > 0)
        if ok.any():
            margin = min(margin, float(np.abs(p_cut[ok] / thr[ok] - 1.0).min()))
        dets.append(d + np.array([[first_row - 1], [first_col - 1]]))
        pows.append(p_cut[hit])
        ratios.append(p_cut[hit] / thr[hit])
    return SimpleNamespace(detections=dets, det_pow=pows, det_ratio=ratios, margin_det=margin, offsets=np.cumsum([0] + [d.shape[1] for d in dets]))


# ---------------------------------------------------------------- step 4
def max_map(P):
    """(M, b*): the maximum over the planes and its first plane in ascending order; a NaN never wins, M is NaN only where every plane is."""
    M = P[:, :, 0].copy()
    arg = np.zeros(M.shape, dtype=np.int64)
    for b in range(1, P.shape[2]):
        v = P[:, :, b]
        with np.errstate(invalid="ignore"):
            take = (v > M) | (np.isnan(M) & ~np.isnan(v))
        M = np.where(take, v, M)
        arg = np.where(take, b, arg)
    return M, arg


def beam_cells(P, dets, first_row, first_col, rect, n_ifft):
    """Step 4 on beam planes P and per-beam lists: rows / cols (1-based rdm bins), hits, power = M, beam (1-based), the margins; sorted by M descending, ties by
    ascending r + nIFFT (c - 1)."""
    row0, row1, col0, col1 = rect
    if row0 - first_row < 1 or col0 - first_col < 1 or row1 - first_row + 1 >= P.shape[0] or col1 - first_col + 1 >= P.shape[1]:
        raise ValueError("the window carries no halo around the CUT zone")
    M, arg = max_map(P)
    H = T.hits_map(dets, M.shape, first_row, first_col)
    rows, cols, hits, power, beam, m_max, m_beam = [], [], [], [], [], [], []
    near = math.inf
    for j, i in zip(*np.nonzero(H.T >= 1)):                        # column first, then row: CUT order
        r, c = i + first_row, j + first_col
        if not (row0 <= r <= row1 and col0 <= c <= col1):
            continue
        nb = M[i - 1:i + 2, j - 1:j + 2].copy()
        v = nb[1, 1]
        nb[1, 1] = -np.inf
        big = nb.max() if not np.isnan(nb).any() else np.nan
        if v > big:                                                # strictly greater than all 8 neighbours; NaN compares false
            others = P[i, j, :][P[i, j, :] != v]
            others = others[~np.isnan(others)]
            rows.append(r); cols.append(c); hits.append(int(H[i, j])); power.append(v); beam.append(int(arg[i, j]) + 1)
            m_max.append((v - big) / v)
            m_beam.append((v - others.max()) / v if others.size else 1.0)
        elif np.isfinite(v) and np.isfinite(big) and big > 0:
            near = min(near, (big - v) / big)
    rows, cols, hits, beam = (np.array(x, dtype=np.int64) for x in (rows, cols, hits, beam))
    power, m_max, m_beam = (np.array(x, dtype=np.float64) for x in (power, m_max, m_beam))
    order = np.lexsort((rows + n_ifft * (cols - 1), -power))
    return SimpleNamespace(row=rows[order], col=cols[order], hits=hits[order], power=power[order], beam=beam[order], margin_max=m_max[order], margin_beam=m_beam[order],
                           near_miss=near, M=M, H=H)


def beam_detect_on_planes(P, first_row, first_col, rect, guard, train, method, alpha, rank, rp):
    """Steps 3 and 4 on given beam planes (the device's own, in the kernel-level test)."""
    d = detect_planes(P, first_row, first_col, rect, guard, train, method, alpha, rank)
    t = beam_cells(P, d.detections, first_row, first_col, rect, int(rp.nIFFT))
    t.rng = (t.row - 1) * rp.rRes                                  # fft2D.m:77,:81
    t.vel = (t.col - int(rp.nFFT) / 2 - 1) * rp.vRes               # fft2D.m:78,:82
    for k in ("detections", "det_pow", "det_ratio", "margin_det", "offsets"):
        setattr(t, k, getattr(d, k))
    return t


def beam_detect(Y, W, first_row, first_col, rect, guard, train, method, rank, rp):
    """Steps 2-4 on a complex window, with the 'Auto' factor of the method at rp.Pfa."""
    alpha = C.threshold_factor(method, C.n_train(guard, train), float(rp.Pfa), rank)
    P = beam_planes(Y, W)
    t = beam_detect_on_planes(P, first_row, first_col, rect, guard, train, method, alpha, rank, rp)
    t.beam_pow, t.alpha = P, alpha
    return t


def margins(t):
    """Every margin of every reported decision of a result, as one array."""
    return np.concatenate([[t.margin_det, t.near_miss], t.margin_max, t.margin_beam])


# ---------------------------------------------------------------- scenes
# the four of the target list (A = 4 and 8, doppler_fft256_kernel, the generic Doppler route zero-padded and truncated), A = 6 (no multiple of 4) and A = 16 at 24 PRB,
# one 2 x 4 planar array, and the weak-target scene: a8_273prb with the second target's echo amplitude x 0.1 -- largeScaleFading is proportional to sqrt(rcs)
# (radarParams.m:49), so rcs = 0.01
WEAK = "a8_273prb_weak"
SCENES = {
    **{k: dict(kind="ula", **v) for k, v in T.SCENES.items()},
    "a6_24prb": dict(kind="ula", n_ants=6, n_slots=2, nrb=24, num_slots_param=6, seed=26, **T._TWO24),
    "a16_24prb": dict(kind="ula", n_ants=16, n_slots=2, nrb=24, num_slots_param=6, seed=27, **T._TWO24),
    "upa2x4_24prb": dict(kind="upa", **U.SCENES["upa2x4_24prb"]),
    WEAK: dict(kind="ula", rcs=(1.0, 0.01), **T.SCENES["a8_273prb"]),
}
GUARD, TRAIN = C.GUARD, C.TRAIN                                    # cfar2D.m:32-33: every scene but T.BAND_SCENE


def bands_of(name):
    """(guard, train) of a scene: T.READER_BANDS for T.BAND_SCENE, (GUARD, TRAIN) for every other one."""
    return T.bands_of(name)


@functools.lru_cache(maxsize=None)
def make(name):
    """The scene; sc.rp is the oracle's radarParams for it.  Shared: callers must not modify it."""
    from conftest import make_scene
    kw = dict(SCENES[name])
    kind, rcs = kw.pop("kind"), kw.pop("rcs", None)
    if kind == "upa":
        n_v, n_h = kw.pop("nV"), kw.pop("nH")
        sc = make_scene(n_ants=n_v * n_h, **kw)
        sc.cell.gNBSenAntenna = SimpleNamespace(kind="upa", nV=n_v, nH=n_h, dV=0.5, dH=0.5)
    else:
        sc = make_scene(**kw)
    if rcs is not None:
        sc.cell.rcs = np.asarray(rcs, dtype=np.float64)
    if kind == "upa" or rcs is not None:
        sc.rp = O.radar_params(sc.cell, sc.carrier, sc.wave)
    return sc


def target_direction(sc, q):
    """(azimuth, elevation) in degrees of target q as radarParams.m:12-14 forms them."""
    x, y, z = np.asarray(sc.cell.targetPosition, dtype=np.float64)[q] - np.asarray(sc.cell.gNBPosition, dtype=np.float64)
    return float(np.rad2deg(np.arctan2(y, x))), float(np.rad2deg(np.arctan2(z, np.hypot(x, y))))


# ---------------------------------------------------------------- beam sets: (azimuths, elevations) in degrees
def beam_set(sc, name):
    a0, e0 = target_direction(sc, 0)
    a1, e1 = target_direction(sc, 1) if int(sc.cell.numTargets) > 1 else (a0, e0)
    if name == "b1":                                               # matched to target 1
        azi, ele = [a0], [e0]
    elif name == "b1_t2":                                          # matched to target 2
        azi, ele = [a1], [e1]
    elif name == "b5":
        azi, ele = [-60.0, a1, 0.0, a0, 45.0], [e0, e1, e0, e0, e1]
    elif name == "b16":
        azi = list(np.arange(16) * 11.0 - 80.0)
        ele = [e0] * 16
    elif name == "b37":                                            # every 10 degrees of the ULA scan grid
        azi = list(np.arange(37) * 10.0 - 180.0)
        ele = [e0] * 37
    elif name == "b361":                                           # the whole scan grid
        azi = list(np.arange(361) * 1.0 - 180.0)
        ele = [e0] * 361
    else:
        raise ValueError(name)
    return np.asarray(azi, dtype=np.float64), np.asarray(ele, dtype=np.float64)


def weights(sc, name):
    """W [A x B] of a beam set through the product's host-side sensing.estimation.beamWeights (NumPy only: no library, no GPU) on the oracle's radarParams."""
    from conftest import load_pkg
    azi, ele = beam_set(sc, name)
    return load_pkg().sensing.estimation.beamWeights(sc.rp, azi, ele), azi


# the cases of tests/test_beam_detect_cpu.py (conditioning) and tests/test_gpu_beam_detect.py: (scene, beam set, method, rank).  CA on every scene with every beam set
# size spread over them; GOCA, SOCA and OS (rank 18 of N = 24) on one scene each; the whole scan grid on one 24-PRB scene.
CASES = (
    ("a4_273prb", "b1", "CA", 1), ("a4_273prb", "b37", "CA", 1),
    ("a8_273prb", "b5", "CA", 1), ("a8_273prb", "b16", "GOCA", 1),
    ("a4_24prb_generic", "b16", "CA", 1), ("a4_24prb_generic", "b361", "CA", 1), ("a4_24prb_generic", "b5", "SOCA", 1),
    ("a4_24prb_truncated", "b37", "CA", 1), ("a4_24prb_truncated", "b5", "OS", 18),
    ("a6_24prb", "b5", "CA", 1), ("a6_24prb", "b37", "CA", 1),
    ("a16_24prb", "b1", "CA", 1), ("a16_24prb", "b16", "CA", 1),
    ("upa2x4_24prb", "b5", "CA", 1), ("upa2x4_24prb", "b16", "CA", 1),
    (WEAK, "b1_t2", "CA", 1), (WEAK, "b37", "CA", 1),
    # the asymmetric bands (hr = 4, hc = 5, gr = 1, gc = 3, N = 78): every method, OS at rank 3N/4
    (T.BAND_SCENE, "b5", "CA", 1), (T.BAND_SCENE, "b16", "GOCA", 1), (T.BAND_SCENE, "b5", "SOCA", 1), (T.BAND_SCENE, "b16", "OS", 58),
)


@functools.lru_cache(maxsize=None)
def oracle_window(name):
    """Oracle stages of a scene: the complex window, its geometry, the per-antenna CA detections and their range list.  Computed once and shared; not to be modified."""
    sc = make(name)
    rp = sc.rp
    cf = T.oracle_config(name, rp)
    echo = O.mono_static_sensing(sc.tx_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, sc.noise, nfft=sc.wave.Nfft)
    rdm = O.rdm_explicit(echo, sc.tx_grid, int(rp.nIFFT), int(rp.nFFT))
    dets, all_rng, _ = detect_per_antenna(rdm, cf, rp.rRes, rp.vRes, int(rp.nFFT))
    rect = (cf.rowRange[0], cf.rowRange[1], cf.colRange[0], cf.colRange[1])
    hr, hc = cf.GuardBandSize[0] + cf.TrainingBandSize[0], cf.GuardBandSize[1] + cf.TrainingBandSize[1]
    assert (tuple(cf.GuardBandSize), tuple(cf.TrainingBandSize)) == bands_of(name) and (name == T.BAND_SCENE or bands_of(name) == (GUARD, TRAIN))
    fr, fc = rect[0] - hr, rect[2] - hc
    win = rdm[fr - 1:rect[1] + hr, fc - 1:rect[3] + hc, :].copy()          # the full map is not kept
    return SimpleNamespace(win=win, rect=rect, first_row=fr, first_col=fc, detections=dets, rng_est=np.unique(all_rng), rdm_max=float(np.abs(rdm).max()))


@functools.lru_cache(maxsize=None)
def oracle_beam_detect(name, beams, method, rank):
    """The oracle-only result of a case.  Computed once and shared; callers must not modify it."""
    sc, w = make(name), oracle_window(name)
    W, azi = weights(sc, beams)
    t = beam_detect(w.win, W, w.first_row, w.first_col, w.rect, *bands_of(name), method, rank, sc.rp)
    t.W, t.beam_azi = W, azi
    t.azi = azi[t.beam - 1]
    return t
