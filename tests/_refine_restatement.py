"""NumPy restatement of isac_fft2d_refine_targets (include/isac_refine.h, DESIGN.md section 5 -- project-defined): steps 1-5 on the range rows of listed cells, every
decision margin, and the scenes its tests share.

The range rows come from the oracle as oracle/fft2d.py:rdm_explicit forms them up to, but not including, the symbol ifftshift: y[r, l, a] in natural symbol order.  Steps 1
and 2 run in fp64, step 3 solves P' = 0 by 60 bisection steps in np.longdouble.  Margins: step 2 = the relative gap of the chosen probe to its two neighbours and to the
runner-up local maximum; step 4 = | |nu_i - nu_k| L - merge_tol | of every pair the rule tests; step 5 = |log2(P_i / (margin P_k D^2))| of every pair it tests."""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np
from scipy import fft as sfft

import oracle as O
from oracle.fft2d import detect_per_antenna
from oracle.matlab_compat import kaiser

import _target_list_restatement as T
import _target_list_upa_restatement as TU

N_BISECT = 60
_LD = np.longdouble
_PI_LD = 4 * np.arctan(_LD(1))


def range_rows(rx_grid, tx_grid, n_ifft):
    """rdm_explicit up to the symbol ifftshift: [nIFFT x L x A], natural symbol order."""
    channel = rx_grid * np.conj(tx_grid) * kaiser(rx_grid.shape[0], 3.0)[:, None, None]
    r = sfft.ifft(channel, n=n_ifft, axis=0, workers=-1) * np.sqrt(n_ifft)
    return r * sfft.fftshift(kaiser(n_ifft, 3.0))[:, None, None]


def rdm_of_rows(rows, n_fft):
    """The rest of rdm_explicit: half swap, zero-padded or truncated Doppler FFT, Doppler fftshift."""
    d = sfft.fft(sfft.ifftshift(rows, axes=1), n=n_fft, axis=1, workers=-1) / np.sqrt(n_fft)
    return sfft.fftshift(d, axes=1)


def spectrum(y, nu):
    """X_a(nu) [A] of one row y [L x A], the direct sum in fp64."""
    l = np.arange(y.shape[0], dtype=np.float64)
    return (y * np.exp(1j * (((-2.0 * np.pi) * nu) * l))[:, None]).sum(axis=0)


def power(y, nu, n_fft):
    x = spectrum(y, nu)
    p = 0.0
    for a in range(x.size):                                              # ascending antenna order from 0.0
        p = p + (x[a].real * x[a].real + x[a].imag * x[a].imag)
    return p / n_fft


def _dp_sign_ld(y_ld, l_ld, nu):
    """The sign carrier of P'(nu) in long double: sum_a Im(conj(X_a) D_a), D_a = sum_l l y e^{-2 pi j nu l}  (P' = 4 pi / nFFT times it)."""
    ph = (-2 * _PI_LD * nu) * l_ld
    e = (np.cos(ph) + 1j * np.sin(ph)).astype(np.clongdouble)
    z = y_ld * e[:, None]
    x, d = z.sum(axis=0), (z * l_ld[:, None]).sum(axis=0)
    return (x.real * d.imag - x.imag * d.real).sum()


def dirichlet2(delta, L):
    s = math.sin(math.pi * delta)
    if s == 0.0:
        return 1.0
    d = math.sin(math.pi * delta * L) / (L * s)
    return d * d


def probe_plan(L, n_fft):
    W = max(1.0 / L, 1.0 / n_fft)
    M = 8 if n_fft >= L else -(-8 * L // n_fft)                          # ceil(8 L W)
    return W, M


def refine(Y, row, col, n_fft, v_res, merge_tol=0.5, merge_rows=1, sidelobe_margin=2.0):
    """Steps 1-5 on Y [n x L x A] (entry i's range row), row / col [n] 1-based.  Returns status, parent, sidelobe_of (input indices), nu, vel, power, snapshots [A x n]
    and the margins m2 [n] (inf for status 1), m4, m5 (lists over the tested pairs)."""
    Y = np.asarray(Y, dtype=np.complex128)
    row, col = np.asarray(row, dtype=np.int64), np.asarray(col, dtype=np.int64)
    n, L, A = Y.shape
    W, M = probe_plan(L, n_fft)
    status, nu, pw = np.zeros(n, dtype=np.int64), np.zeros(n), np.zeros(n)
    m2 = np.full(n, np.inf)
    snaps = np.zeros((A, n), dtype=np.complex128)
    l_ld = np.arange(L).astype(_LD)
    for i in range(n):
        nu0 = float(col[i] - n_fft // 2 - 1) / n_fft
        nus = [nu0 + (g * W) / M for g in range(-M, M + 1)]
        P = np.array([power(Y[i], v, n_fft) for v in nus])
        maxima = [g for g in range(1, 2 * M) if P[g] > P[g - 1] and P[g] >= P[g + 1]]
        if not maxima:
            status[i], nu[i] = 1, nu0
        else:
            g = max(maxima, key=lambda q: (P[q], -q))                     # the largest P, the lowest g on a tie
            gaps = [(P[g] - P[g - 1]) / P[g], (P[g] - P[g + 1]) / P[g]] + [abs(P[g] - P[q]) / P[g] for q in maxima if q != g]
            m2[i] = min(gaps)
            y_ld = Y[i].astype(np.clongdouble)
            lo, hi = _LD(nus[g - 1]), _LD(nus[g + 1])
            for _ in range(N_BISECT):
                mid = (lo + hi) / 2
                if _dp_sign_ld(y_ld, l_ld, mid) > 0:
                    lo = mid
                else:
                    hi = mid
            nu[i] = float((lo + hi) / 2)
        pw[i] = power(Y[i], nu[i], n_fft)
        snaps[:, i] = spectrum(Y[i], nu[i]) / np.sqrt(float(n_fft))
    vel = np.where(status == 0, nu * n_fft * v_res, (col - n_fft / 2 - 1) * v_res)
    parent, side = np.arange(n), np.full(n, -1, dtype=np.int64)
    m4, m5 = [], []
    for i in range(n):
        if status[i] or merge_tol == 0:                                   # merge_tol == 0 disables the step
            continue
        for k in range(i):
            if parent[k] == k and status[k] == 0 and abs(row[i] - row[k]) <= merge_rows:
                dist = abs(nu[i] - nu[k]) * L
                m4.append(abs(dist - merge_tol))
                if dist <= merge_tol:
                    parent[i] = k
                    break
    for i in range(n):
        if parent[i] != i or status[i] or sidelobe_margin == 0:
            continue
        for k in range(n):
            if k != i and parent[k] == k and status[k] == 0 and abs(row[i] - row[k]) <= merge_rows and pw[k] > pw[i]:
                bound = sidelobe_margin * pw[k] * dirichlet2(nu[i] - nu[k], L)
                m5.append(abs(math.log2(pw[i] / bound)) if bound > 0 and pw[i] > 0 else math.inf)
                if pw[i] <= bound:
                    side[i] = k
                    break
    return SimpleNamespace(status=status, parent=parent, sidelobe_of=side, nu=nu, vel=vel, power=pw, snapshots=snaps, m2=m2, m4=m4, m5=m5,
                           n_kept=int((parent == np.arange(n)).sum()))


# ---------------------------------------------------------------- the scenes of tests/test_refine_cpu.py (conditioning) and tests/test_gpu_refine.py
# split273*: the 273-PRB scenes of the list with velocities 1.5 and -2.5 nFFT / L bins: the Doppler phase advances by a fraction of a turn over the L symbols and the
# half swap splits the peak.  split24: the same at 24 PRB with nFFT = 64 > L = 28.  The four scenes of the list itself and one planar array.
_SPLIT = dict(n_slots=4, targets=T._POS, velocity=(1.5 * T._V273, -2.5 * T._V273), zero_s_slots=False)
SCENES = {
    "split273": dict(n_ants=4, seed=21, **_SPLIT),
    "split273_a8": dict(n_ants=8, seed=22, **_SPLIT),
    **T.SCENES,
    "split24": dict(n_ants=4, n_slots=2, nrb=24, num_slots_param=6, seed=23, targets=T._POS, velocity=(30.0, -45.0), zero_s_slots=False),
    "upa2x2_24prb": None,                                                # tests/_target_list_upa_restatement.py
    "upa8x16_24prb": None,                                               # ... A = 128: more antennas than the 64 quads of a workgroup, the kernel's second pass
}
MIN_ENTRIES = {"upa8x16_24prb": 1}                                      # entries the list must hold (default 2, one per target): with 128 elements only the stronger target is listed
SPLIT_LOBES =((88, 133), (88, 139))                                     # split273: the two lobes of the stronger target's tone


def is_upa(name):
    return SCENES[name] is None


def make(name):
    if is_upa(name):
        return TU.make(name)
    from conftest import make_scene
    return make_scene(**SCENES[name])


@functools.lru_cache(maxsize=None)
def oracle_scene(name):
    """Oracle only: O.mono_static_sensing -> the range rows -> rdm -> the oracle CFAR -> the list's cells (tests/_target_list_restatement.py: target_cells) -> refine.
    Computed once per scene and shared; callers must not modify it.  Only the rows of the window are kept (``rows_of``)."""
    sc = make(name)
    rp = sc.rp
    cf = T.oracle_config(name, rp)                                        # the default bands for every scene but T.BAND_SCENE
    n_ifft, n_fft = int(rp.nIFFT), int(rp.nFFT)
    echo = O.mono_static_sensing(sc.tx_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, sc.noise, nfft=sc.wave.Nfft)
    rows = range_rows(echo, sc.tx_grid, n_ifft)
    rect = (cf.rowRange[0], cf.rowRange[1], cf.colRange[0], cf.colRange[1])
    hr, hc = cf.GuardBandSize[0] + cf.TrainingBandSize[0], cf.GuardBandSize[1] + cf.TrainingBandSize[1]
    fr, fc = rect[0] - hr, rect[2] - hc
    rows = rows[fr - 1:rect[1] + hr].copy()                               # window rows only
    rdm = rdm_of_rows(rows, n_fft)                                        # [nr x nFFT x A]
    full = np.zeros((n_ifft,) + rdm.shape[1:], dtype=np.complex128)      # (the detector takes map coordinates; it reads the window only)
    full[fr - 1:rect[1] + hr] = rdm
    dets, _, _ = detect_per_antenna(full, cf, rp.rRes, rp.vRes, n_fft)
    win = rdm[:, fc - 1:rect[3] + hc, :]
    t = T.target_cells(np.abs(win) ** 2, dets, fr, fc, rect, n_ifft)
    s = SimpleNamespace(sc=sc, rp=rp, L=rows.shape[1], n_fft=n_fft, first_row=fr, rect=rect, row=t.row, col=t.col, rng=(t.row - 1) * rp.rRes,
                        grid_vel=(t.col - n_fft / 2 - 1) * rp.vRes)
    s.rows_of = lambda r: rows[np.asarray(r) - fr]
    s.ref = refine(s.rows_of(t.row), t.row, t.col, n_fft, float(rp.vRes))
    return s


def true_velocity(s, i):
    """The velocity of the first true target within one range resolution cell of entry i's grid range (the matching of getRMSE.m:43), or None."""
    for tgt in s.rp.targetRealPos:
        if abs(float(tgt["Range"]) - s.rng[i]) < s.rp.rRes:
            return float(tgt["Velocity"])
    return None
