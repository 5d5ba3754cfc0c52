"""NumPy restatement of the CA / GOCA / SOCA / OS detectors of include/isac_cfar.h (isac_cfar2d, isac_fft2d_redetect, isac_cfar_threshold_factor; project-defined where
phased.CFARDetector2D's documentation is silent -- DESIGN.md section 5), and what its CPU and GPU tests share.

For a CUT, hr = guard[0] + train[0], hc = guard[1] + train[1]: the training cells T_1 .. T_N are the (2 hr + 1) x (2 hc + 1) window minus the guard block in the order of
oracle/cfar.py (column offset slowest, row offset fastest).  CA: sum / N.  GOCA / SOCA: the front half T_1 .. T_{N/2} and the rest, each summed from 0.0 in order and
divided by N/2; the greater / smaller mean.  OS: the rank-th smallest.  thr = alpha * estimate, detection iff P[cut] > thr; a NaN anywhere gives none."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

from oracle.cfar import cfar_threshold_factor, training_offsets

METHODS = ("CA", "GOCA", "SOCA", "OS")
GUARD_BAND = 1e-9        # the project's own guard band ("no CUT within 1e-9 relative of threshold")


def n_train(guard, train):
    return len(training_offsets(guard, train))


def training_cells(P, cut_idx, guard, train):
    """T [N x nCUT]: the training cells of every CUT (cut_idx [2 x nCUT], 1-based) in the defined order."""
    p = np.asarray(P, dtype=np.float64)
    cut = np.asarray(cut_idx, dtype=np.int64).reshape(2, -1)
    r, c = cut[0] - 1, cut[1] - 1
    hr, hc = guard[0] + train[0], guard[1] + train[1]
    if cut.shape[1] and (r.min() - hr < 0 or r.max() + hr >= p.shape[0] or c.min() - hc < 0 or c.max() + hc >= p.shape[1]):
        raise ValueError("CUT training window exceeds the input matrix")
    return np.stack([p[r + dr, c + dc] for dr, dc in training_offsets(guard, train)])


def _sum_in_order(T):
    acc = np.zeros(T.shape[1], dtype=np.float64)
    for row in T:                                       # left to right from 0.0
        acc = acc + row
    return acc


def noise_estimate(T, method, rank=1):
    """The method's noise estimate from T [N x n]; NaN where any training cell is NaN."""
    N = T.shape[0]
    if method == "CA":
        est = _sum_in_order(T) / N
    elif method in ("GOCA", "SOCA"):
        front, rear = _sum_in_order(T[: N // 2]) / (N // 2), _sum_in_order(T[N // 2:]) / (N // 2)
        est = np.where(front > rear, front, rear) if method == "GOCA" else np.where(front < rear, front, rear)
    elif method == "OS":
        if not 1 <= rank <= N:
            raise ValueError("rank outside 1..N")
        est = np.partition(T, rank - 1, axis=0)[rank - 1]
    else:
        raise ValueError(method)
    return np.where(np.isnan(T).any(axis=0), np.nan, est)


# ---------------------------------------------------------------- ThresholdFactor 'Auto'
def false_alarm(method, N, alpha, rank=1):
    """Left side of the method's false-alarm equation (exponential cells).  The SOCA terms by the ratio recurrence t_{k+1} = t_k (n + k) / ((k + 1)(2 + T))."""
    n, T = N // 2, alpha / (N // 2) if N >= 2 else alpha
    if method == "CA":
        return (1.0 + alpha / N) ** -N
    if method == "OS":
        p = 1.0
        for i in range(rank):
            p *= (N - i) / (N - i + alpha)
        return p
    t, s = (2.0 + T) ** -n, 0.0
    for k in range(n):
        s += t
        t = t * (n + k) / ((k + 1) * (2.0 + T))
    return 2.0 * s if method == "SOCA" else 2.0 * (1.0 + T) ** -n - 2.0 * s


def threshold_factor(method, N, pfa, rank=1):
    """CA: the closed form of oracle/cfar.py.  Otherwise the root of false_alarm(alpha) = pfa: the bracket [0, 1] doubled until it holds the root, halved until its ends
    are adjacent doubles (or 200 times); the upper end."""
    if method == "CA":
        return cfar_threshold_factor(N, pfa)
    lo, hi = 0.0, 1.0
    while false_alarm(method, N, hi, rank) > pfa:
        lo, hi = hi, 2.0 * hi
    for _ in range(200):
        mid = lo + (hi - lo) / 2.0
        if not lo < mid < hi:
            break
        if false_alarm(method, N, mid, rank) > pfa:
            lo = mid
        else:
            hi = mid
    return hi


# ---------------------------------------------------------------- the detector
def detect(P, cut_idx, guard, train, method, alpha, rank=1, return_threshold=False):
    """[2 x D] 1-based detections in CUT-list order (and the per-CUT thresholds)."""
    cut = np.asarray(cut_idx, dtype=np.int64).reshape(2, -1)
    thr = alpha * noise_estimate(training_cells(P, cut, guard, train), method, rank)
    det = np.asarray(P, dtype=np.float64)[cut[0] - 1, cut[1] - 1] > thr          # strict; NaN compares false
    return (cut[:, det], thr) if return_threshold else cut[:, det]


def rectangle_cuts(rect):
    """The rows-fastest CUT list of the rectangle (row0, row1, col0, col1), 1-based inclusive (cfar2D.m:23-24)."""
    row0, row1, col0, col1 = rect
    cc, rr = np.meshgrid(np.arange(col0, col1 + 1), np.arange(row0, row1 + 1))
    return np.stack([rr.ravel(order="F"), cc.ravel(order="F")]).astype(np.int64)


def unique_stable(v):
    _, first = np.unique(v, return_index=True)
    return np.asarray(v)[np.sort(first)]


def redetect(P, first_row, first_col, rect, guard, train, method, alpha, rank, r_res, v_res, n_fft, return_margin=False):
    """isac_fft2d_redetect on a power window P [nr x nc x A] whose cell (0, 0) is rdm cell (first_row, first_col): the per-antenna lists in rdm coordinates with the CUTs'
    powers, and the host half of fft2D.m:63-99 on them (peak sort per antenna, concatenation, the two unique(., 'stable')).  ``margin``: the smallest |P - thr| / thr
    over every CUT of every antenna with a finite positive threshold."""
    cuts = rectangle_cuts(rect)
    local = cuts - np.array([[first_row - 1], [first_col - 1]])
    dets, pows, rows, cols, margin = [], [], [], [], np.inf
    for a in range(P.shape[2]):
        d, thr = detect(P[:, :, a], local, guard, train, method, alpha, rank, return_threshold=True)
        pw = P[d[0] - 1, d[1] - 1, a]
        d = d + np.array([[first_row - 1], [first_col - 1]])
        order = np.argsort(-pw, kind="stable")                                # fft2D.m:89 sort(peaks, 'descend')
        rows.append(d[0][order]); cols.append(d[1][order])
        dets.append(d); pows.append(pw)
        ok = np.isfinite(thr) & (thr > 0)
        if ok.any():
            margin = min(margin, float((np.abs(P[local[0] - 1, local[1] - 1, a][ok] - thr[ok]) / thr[ok]).min()))
    urow, ucol = unique_stable(np.concatenate(rows)), unique_stable(np.concatenate(cols))
    out = SimpleNamespace(detections=dets, det_pow=pows, rngEst=(urow - 1) * r_res, velEst=(ucol - n_fft / 2 - 1) * v_res, numDets=int(urow.size),
                          totalDetections=int(sum(d.shape[1] for d in dets)), offsets=np.cumsum([0] + [d.shape[1] for d in dets]))
    if return_margin:
        out.margin = margin
    return out


# ---------------------------------------------------------------- what the GPU chain test compares with: the oracle-only result of every scene x method pair
GUARD, TRAIN = (2, 2), (1, 1)                                                  # cfar2D.m:32-33
CHAIN_METHODS = (("CA", 1), ("GOCA", 1), ("SOCA", 1), ("OS", 18))              # N = 24; rank 18 = 3N/4


def chain_methods(name):
    """CHAIN_METHODS at the scene's bands (tests/_target_list_restatement.py: bands_of): the OS rank is 3N/4 of the scene's N, 18 of 24 at the default bands."""
    import _target_list_restatement as R
    n = n_train(*R.bands_of(name))
    return tuple((m, 3 * n // 4 if m == "OS" else k) for m, k in CHAIN_METHODS)


@functools.lru_cache(maxsize=None)
def oracle_redetect(name, method, rank):
    """Oracle chain (tests/_target_list_restatement.py: oracle_targets) -> |rdm|^2 window -> the restatement.  Computed once and shared; callers must not modify it."""
    import _target_list_restatement as R
    t = R.oracle_targets(name)
    rp = R.make(name).rp
    nr, nc = t.S.shape
    rr, cc = np.arange(t.first_row, t.first_row + nr), np.arange(t.first_col, t.first_col + nc)
    win = np.transpose(t.rdm_at(rr[:, None], cc[None, :]), (2, 1, 0))          # rdm_at gives [A x nc x nr]
    guard, train = R.bands_of(name)
    alpha = threshold_factor(method, n_train(guard, train), float(rp.Pfa), rank)
    return redetect(np.abs(win) ** 2, t.first_row, t.first_col, t.rect, guard, train, method, alpha, rank, rp.rRes, rp.vRes, int(rp.nFFT), return_margin=True)


def chain_pairs():
    """(cleared, dropped): the scene x method pairs whose every CUT on the oracle's power window lies more than GUARD_BAND (relative) away from its threshold, and the rest."""
    import _target_list_restatement as R
    cleared, dropped = [], []
    for name in R.SCENES:
        for method, rank in chain_methods(name):
            (cleared if oracle_redetect(name, method, rank).margin > GUARD_BAND else dropped).append((name, method, rank))
    return cleared, dropped
