"""NumPy restatement of isac_fft2d_clean_targets (include/isac_clean.h, DESIGN.md section 5 -- project-defined): the loop of successive cancellation on the range rows of
a CPI, every decision margin per pass, and the scenes its tests share.

Built on the parts the loop is made of: the range rows and the map of tests/_refine_restatement.py (range_rows, rdm_of_rows, refine), the detector of
tests/_cfar_methods_restatement.py through tests/_beam_detect_restatement.py:detect_planes, the cells of tests/_target_list_restatement.py:target_cells.  Step 8 -- the fit of
the tone over the active symbols and its subtraction -- runs in np.longdouble and is rounded to fp64 once per pass.  Margins per pass: ``det`` = the smallest |P / thr - 1|
over every CUT of every antenna plane, ``max`` = the smallest relative lead of a listed cell over its largest neighbour, ``near`` = the smallest relative shortfall of a
detected CUT cell that is not listed, ``m2`` = step 2 of the refinement, ``parent`` = | |nu_i - nu_k| L - merge_tol | of every pair step 7 tests."""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np

import oracle as O
from oracle.fft2d import detect_per_antenna

import _beam_detect_restatement as B
import _cfar_methods_restatement as C
import _refine_restatement as R
import _target_list_restatement as T

_LD = np.longdouble
_PI_LD = 4 * np.arctan(_LD(1))
MAX_ITER = 8           # what the tests run the loop with unless a case says otherwise: every scene is exhausted (n_left = 0) before that


def cancel_ld(y, nu, active):
    """Step 8 on one row y [L x A] (any float type) in long double: y - c e^{+2 pi j nu l} on the active symbols, c = mean over them of y e^{-2 pi j nu l}."""
    y = np.asarray(y).astype(np.clongdouble)
    act = np.flatnonzero(active)
    ph = (-2 * _PI_LD * _LD(nu)) * act.astype(_LD)
    e = (np.cos(ph) + 1j * np.sin(ph)).astype(np.clongdouble)
    c = (y[act] * e[:, None]).sum(axis=0) / _LD(act.size)
    y[act] = y[act] - c[None, :] * np.conj(e)[:, None]
    return y


def span_of(row, first_row, n_rows, span_rows):
    """The 0-based window rows |r' - r| <= span_rows, clipped to the window."""
    wr = int(row) - first_row
    return range(max(wr - span_rows, 0), min(wr + span_rows, n_rows - 1) + 1)


def cells_of_rows(rows, g, method="CA", rank=1, alpha=None):
    """Steps 1-3 on rows [nr x L x A]: the list's cells with the pass's margins."""
    win = R.rdm_of_rows(rows, g.n_fft)[:, g.first_col - 1:g.rect[3] + g.hc, :]
    P = win.real * win.real + win.imag * win.imag                           # two products, one sum
    if alpha is None:
        alpha = C.threshold_factor(method, C.n_train(g.guard, g.train), g.pfa, rank)
    d = B.detect_planes(P, g.first_row, g.first_col, g.rect, g.guard, g.train, method, alpha, rank)
    t = T.target_cells(P, d.detections, g.first_row, g.first_col, g.rect, g.n_ifft)
    t.margin_det = d.margin_det
    return t


def clean(rows, g, max_iter=MAX_ITER, span_rows=2, merge_tol=0.5, method="CA", rank=1, alpha=None, sym_active=None):
    """The loop on rows [nr x L x A] (window row 0 = map row g.first_row, 1-based) with the geometry g of ``geometry``.  Returns the entries, n_iter / n_kept / n_left, the
    residual rows and ``margins``: one namespace (det, max, near, m2, parent) per pass that ran steps 1-3; ``lists``: the (row, col) list of every such pass."""
    Rr = np.array(rows, dtype=np.complex128)
    nr, L, A = Rr.shape
    active = np.ones(L, dtype=bool) if sym_active is None else np.asarray(sym_active).astype(bool)
    if not active.any():
        raise ValueError("no active symbol")
    e = SimpleNamespace(row=[], col=[], hits=[], status=[], parent=[], map_power=[], nu=[], vel=[], rng=[], power=[], snapshots=[])
    margins, lists = [], []
    n_left = 0
    i = 0
    while True:
        t = cells_of_rows(Rr, g, method, rank, alpha)
        m = SimpleNamespace(det=t.margin_det, max=float(t.margin1.min()) if t.row.size else math.inf, near=t.near_miss, m2=math.inf, parent=math.inf)
        margins.append(m)
        lists.append(list(zip(t.row.tolist(), t.col.tolist())))
        n_left = int(t.row.size)
        if n_left == 0 or i == max_iter:
            break
        r, c = int(t.row[0]), int(t.col[0])
        y = Rr[r - g.first_row]
        f = R.refine(y[None], [r], [c], g.n_fft, g.v_res, merge_tol=0.0, sidelobe_margin=0.0)
        m.m2 = float(f.m2[0])
        e.row.append(r); e.col.append(c); e.hits.append(int(t.hits[0])); e.map_power.append(float(t.power[0])); e.rng.append((r - 1) * g.r_res)
        e.status.append(int(f.status[0])); e.nu.append(float(f.nu[0])); e.vel.append(float(f.vel[0])); e.power.append(float(f.power[0])); e.snapshots.append(f.snapshots[:, 0])
        parent = i
        if f.status[0] == 0 and merge_tol != 0:
            for k in range(i):
                if e.parent[k] == k and abs(r - e.row[k]) <= span_rows:
                    dist = abs(e.nu[i] - e.nu[k]) * L
                    m.parent = min(m.parent, abs(dist - merge_tol))
                    if dist <= merge_tol:
                        parent = k
                        break
        e.parent.append(parent)
        i += 1
        if f.status[0] != 0:
            break
        for wr in span_of(r, g.first_row, nr, span_rows):
            Rr[wr] = cancel_ld(Rr[wr], e.nu[-1], active).astype(np.complex128)
    out = SimpleNamespace(**{k: np.array(v, dtype=np.int64 if k in ("row", "col", "hits", "status", "parent") else np.float64) for k, v in vars(e).items() if k != "snapshots"})
    out.snapshots = np.stack(e.snapshots, axis=1) if e.snapshots else np.zeros((A, 0), dtype=np.complex128)
    out.n_iter, out.n_left, out.n_kept = i, n_left, int(sum(p == j for j, p in enumerate(e.parent)))
    out.residual, out.margins, out.lists = Rr, margins, lists
    return out


def min_margin(res):
    """The smallest margin of any decision of any pass."""
    return min(min(m.det, m.max, m.near, m.m2, m.parent) for m in res.margins)


def replay(rows, g, row, nu, span_rows, sym_active=None):
    """Step 8 alone, in long double throughout, for a given (row, nu) sequence: what the residual rows should be."""
    Rr = np.asarray(rows).astype(np.clongdouble)
    active = np.ones(Rr.shape[1], dtype=bool) if sym_active is None else np.asarray(sym_active).astype(bool)
    for r, v in zip(row, nu):
        for wr in span_of(r, g.first_row, Rr.shape[0], span_rows):
            Rr[wr] = cancel_ld(Rr[wr], v, active)
    return Rr


# ---------------------------------------------------------------- scenes
# masked: a4_273prb with BOTH targets at 100 m (+-20 m across), velocities +-_V273, the second one's echo amplitude x 0.1 (rcs 0.01): its cell lies under the first one's
# Doppler sidelobes and fails the detector.  masked_gap: the same with the 'S' slot (symbols 42 .. 55 of 56) silent.  The rest: tests/_refine_restatement.py.
_MASKED = dict(n_ants=4, n_slots=4, seed=21, targets=((100.0, 20.0, 1.5), (100.0, -20.0, 1.5)), velocity=(T._V273, -T._V273))
OWN = {"masked": dict(zero_s_slots=False, **_MASKED), "masked_gap": dict(zero_s_slots=True, **_MASKED)}
RCS = (1.0, 0.01)
# BANDS_SCENE: "masked" once more (another seed) at the asymmetric guard / training bands T.READER_BANDS -- the passes' detector, their list and the rows they cancel on all
# take the window's geometry (hr = 4 rows, hc = 5 columns around the CUT zone, a 3 x 7 guard block) from the CPI
BANDS_SCENE = "masked_g13_t32"
OWN[BANDS_SCENE] = dict(zero_s_slots=False, **{**_MASKED, "seed": 27})
T.BANDS[BANDS_SCENE] = T.READER_BANDS
SCENES = ("masked", "masked_gap", "split273", "a4_273prb", "a8_273prb", "a4_24prb_generic", "a4_24prb_truncated", "split24", "upa2x2_24prb", "upa8x16_24prb", BANDS_SCENE)
MASKED_CELL = (88, 124)                                                    # the weak target's cell
GAP_MASK = np.r_[np.ones(42, dtype=np.uint8), np.zeros(14, dtype=np.uint8)]
# the cases of tests/test_clean_cpu.py and tests/test_gpu_clean.py: name -> (scene, keywords of ``clean``)
CASES = {**{s: (s, {}) for s in SCENES if s != "masked_gap"},
         "masked_gap": ("masked_gap", dict(sym_active=GAP_MASK)), "masked_gap_nomask": ("masked_gap", {}),
         "masked_span0": ("masked", dict(span_rows=0)), "masked_span1": ("masked", dict(span_rows=1)),
         "masked_bigtol": ("masked", dict(merge_tol=1e6)),                  # the second entry lies 1.96 / L from the first: a tolerance that wide makes it a residue (step 7 taken)
         "masked_tol0": ("masked", dict(merge_tol=0.0)),                    # step 7 switched off
         "split273_one": ("split273", dict(max_iter=1)),                    # the closing pass after max_iter entries: n_left = the 3 cells of the second pass's list
         BANDS_SCENE + "_goca": (BANDS_SCENE, dict(method="GOCA")), BANDS_SCENE + "_soca": (BANDS_SCENE, dict(method="SOCA")),
         BANDS_SCENE + "_os": (BANDS_SCENE, dict(method="OS", rank=58)),      # rank 3N/4 of the N = 78 training cells
         "masked_goca": ("masked", dict(method="GOCA")), "split24_soca": ("split24", dict(method="SOCA")), "a4_24prb_generic_os": ("a4_24prb_generic", dict(method="OS", rank=18))}


def is_upa(scene):
    return scene.startswith("upa")


@functools.lru_cache(maxsize=None)
def make(scene):
    """The scene; sc.rp is the oracle's radarParams for it.  Shared: callers must not modify it."""
    if scene not in OWN:
        return R.make(scene)
    from conftest import make_scene
    sc = make_scene(**OWN[scene])
    sc.cell.rcs = np.asarray(RCS, dtype=np.float64)
    sc.rp = O.radar_params(sc.cell, sc.carrier, sc.wave)
    return sc


def geometry(rp, cf):
    rect = (cf.rowRange[0], cf.rowRange[1], cf.colRange[0], cf.colRange[1])
    guard, train = tuple(cf.GuardBandSize), tuple(cf.TrainingBandSize)
    hr, hc = guard[0] + train[0], guard[1] + train[1]
    return SimpleNamespace(rect=rect, guard=guard, train=train, hr=hr, hc=hc, first_row=rect[0] - hr, first_col=rect[2] - hc, n_rows=rect[1] - rect[0] + 1 + 2 * hr,
                           n_fft=int(rp.nFFT), n_ifft=int(rp.nIFFT), pfa=float(rp.Pfa), r_res=float(rp.rRes), v_res=float(rp.vRes))


@functools.lru_cache(maxsize=None)
def oracle_rows(scene):
    """Oracle only: O.mono_static_sensing -> the window's range rows, the geometry, and the list of the CPI (the oracle's per-antenna CA-CFAR on the oracle's map -> the
    list's cells), as tests/_refine_restatement.py:oracle_scene forms it.  Computed once per scene and shared; callers must not modify it."""
    sc = make(scene)
    rp = sc.rp
    cf = T.oracle_config(scene, rp)                                        # the default bands for every scene but BANDS_SCENE
    g = geometry(rp, cf)
    echo = O.mono_static_sensing(sc.tx_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, sc.noise, nfft=sc.wave.Nfft)
    rows = R.range_rows(echo, sc.tx_grid, g.n_ifft)[g.first_row - 1:g.first_row - 1 + g.n_rows].copy()
    rdm = R.rdm_of_rows(rows, g.n_fft)
    full = np.zeros((g.n_ifft,) + rdm.shape[1:], dtype=np.complex128)      # (the detector takes map coordinates; it reads the window only)
    full[g.first_row - 1:g.first_row - 1 + g.n_rows] = rdm
    dets, _, _ = detect_per_antenna(full, cf, rp.rRes, rp.vRes, g.n_fft)
    win = rdm[:, g.first_col - 1:g.rect[3] + g.hc, :]
    lst = T.target_cells(np.abs(win) ** 2, dets, g.first_row, g.first_col, g.rect, g.n_ifft)
    return SimpleNamespace(sc=sc, rp=rp, g=g, rows=rows, L=rows.shape[1], list=lst, cells=list(zip(lst.row.tolist(), lst.col.tolist())))


@functools.lru_cache(maxsize=None)
def oracle_clean(case):
    """The oracle-only result of a case.  Computed once and shared; callers must not modify it."""
    scene, kw = CASES[case]
    s = oracle_rows(scene)
    return clean(s.rows, s.g, **kw)


def true_velocity(rp, q):
    return float(rp.targetRealPos[q]["Velocity"])
