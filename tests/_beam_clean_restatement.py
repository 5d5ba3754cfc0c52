"""NumPy restatement of isac_fft2d_beam_clean_targets (include/isac_beam_clean.h, DESIGN.md section 5 -- project-defined): the loop of successive cancellation with the
detector on beam planes, every decision margin per pass, and the scenes, beam sets and cases its tests share.

Built from the parts the committed restatements hold: the map of tests/_refine_restatement.py (rdm_of_rows) and its refinement (refine), the beam planes and steps 3-4 of
tests/_beam_detect_restatement.py (beam_planes, beam_detect_on_planes), step 8 and the row span of tests/_clean_restatement.py (cancel_ld, span_of).  The loop recomputes the
whole window in every pass -- the definition; the band update is the library's business.  Margins per pass: ``det`` = the smallest |P / thr - 1| over every CUT of every
beam plane, ``max`` = the smallest relative lead of a listed cell over its largest neighbour, ``near`` = the smallest relative shortfall of a detected CUT cell that is not
listed, ``order`` = the smallest relative gap between two consecutive cells of the list, ``beam`` = how far M of the picked cell lies above the next beam's value, ``m2`` =
step 2 of the refinement, ``parent`` = | |nu_i - nu_k| L - merge_tol | of every pair the parent step tests."""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np

import oracle as O

import _beam_detect_restatement as B
import _cfar_methods_restatement as C
import _clean_restatement as K
import _refine_restatement as R
import _target_list_restatement as T

MAX_ITER = 8           # what the tests run the loop with unless a case says otherwise
MARGIN_KEYS = ("det", "max", "near", "order", "beam", "m2", "parent")


def planes_of_rows(rows, g, W):
    """Step 1 on rows [nr x L x A]: the beam planes [nr x nc x B] of the window."""
    win = R.rdm_of_rows(rows, g.n_fft)[:, g.first_col - 1:g.rect[3] + g.hc, :]
    return B.beam_planes(win, W)


def cells_of_planes(P, g, method="CA", rank=1, alpha=None):
    """Steps 2 and 3 on beam planes: the list's cells (B.beam_detect_on_planes) with ``margin_order`` added."""
    if alpha is None:
        alpha = C.threshold_factor(method, C.n_train(g.guard, g.train), g.pfa, rank)
    rp = SimpleNamespace(nIFFT=g.n_ifft, nFFT=g.n_fft, rRes=g.r_res, vRes=g.v_res)
    t = B.beam_detect_on_planes(P, g.first_row, g.first_col, g.rect, g.guard, g.train, method, alpha, rank, rp)
    t.margin_order = float(((t.power[:-1] - t.power[1:]) / t.power[:-1]).min()) if t.row.size > 1 else math.inf
    return t


def beam_clean(rows, g, W, beam_azi=None, max_iter=MAX_ITER, span_rows=2, merge_tol=0.5, method="CA", rank=1, alpha=None, sym_active=None):
    """The loop on rows [nr x L x A] (window row 0 = map row g.first_row, 1-based) with the geometry g of K.geometry and the weights W [A x B].  Returns the entries,
    n_iter / n_kept / n_left, the residual rows, ``beam_pow`` and ``left_cells`` of the last run of steps 1-3, ``margins`` (one namespace per such run) and ``lists``."""
    Rr = np.array(rows, dtype=np.complex128)
    nr, L, A = Rr.shape
    active = np.ones(L, dtype=bool) if sym_active is None else np.asarray(sym_active).astype(bool)
    if not active.any():
        raise ValueError("no active symbol")
    e = SimpleNamespace(row=[], col=[], hits=[], beam=[], status=[], parent=[], map_power=[], nu=[], vel=[], rng=[], power=[], beam_label=[], snapshots=[])
    margins, lists = [], []
    i = 0
    while True:
        P = planes_of_rows(Rr, g, W)
        t = cells_of_planes(P, g, method, rank, alpha)
        m = SimpleNamespace(det=t.margin_det, max=float(t.margin_max.min()) if t.row.size else math.inf, near=t.near_miss, order=t.margin_order, beam=math.inf, m2=math.inf,
                            parent=math.inf)
        margins.append(m)
        lists.append(list(zip(t.row.tolist(), t.col.tolist())))
        n_left = int(t.row.size)
        if n_left == 0 or i == max_iter:
            break
        r, c, b = int(t.row[0]), int(t.col[0]), int(t.beam[0])
        m.beam = float(t.margin_beam[0])
        f = R.refine(Rr[r - g.first_row][None], [r], [c], g.n_fft, g.v_res, merge_tol=0.0, sidelobe_margin=0.0)
        m.m2 = float(f.m2[0])
        e.row.append(r); e.col.append(c); e.hits.append(int(t.hits[0])); e.beam.append(b); e.map_power.append(float(t.power[0])); e.rng.append((r - 1) * g.r_res)
        e.beam_label.append(float(b) if beam_azi is None else float(beam_azi[b - 1]))
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
        for wr in K.span_of(r, g.first_row, nr, span_rows):
            Rr[wr] = K.cancel_ld(Rr[wr], e.nu[-1], active).astype(np.complex128)
    ints = ("row", "col", "hits", "beam", "status", "parent")
    out = SimpleNamespace(**{k: np.array(v, dtype=np.int64 if k in ints else np.float64) for k, v in vars(e).items() if k != "snapshots"})
    out.snapshots = np.stack(e.snapshots, axis=1) if e.snapshots else np.zeros((A, 0), dtype=np.complex128)
    out.n_iter, out.n_left, out.n_kept = i, n_left, int(sum(p == j for j, p in enumerate(e.parent)))
    out.residual, out.beam_pow, out.left_cells, out.margins, out.lists = Rr, P, np.array(lists[-1], dtype=np.int64).reshape(-1, 2), margins, lists
    return out


def min_margin(res):
    """The smallest margin of any decision of any pass."""
    return min(min(getattr(m, k) for k in MARGIN_KEYS) for m in res.margins)


def touched_rows(res, g, span_rows):
    """The 0-based window rows inside the band of any subtraction of a result (an entry with status 1 subtracts nothing)."""
    return sorted({wr for r, st in zip(res.row.tolist(), res.status.tolist()) if st == 0 for wr in K.span_of(r, g.first_row, g.n_rows, span_rows)})


# ---------------------------------------------------------------- scenes
# cap8: the scene of the capability test -- K's ``masked`` with 8 elements and the second echo 30 dB down (rcs 0.001): cleanTargets has no array gain and beamDetect reads one
# map, so neither lists the weak target's cell (88, 124); the loop does.  cap8_s22 / cap8_s23: the same with other noise and data seeds (tests/test_beam_clean_cpu.py only).
# Every other scene is one of tests/_clean_restatement.py or tests/_beam_detect_restatement.py.
CAP, CAP_RCS, CAP_CELLS = "cap8", (1.0, 0.001), [(88, 134), (88, 124)]
_CAP = {CAP: 21, "cap8_s22": 22, "cap8_s23": 23}
GAP_MASK = K.GAP_MASK


@functools.lru_cache(maxsize=None)
def make(scene):
    """The scene; sc.rp is the oracle's radarParams for it.  Shared: callers must not modify it."""
    if scene in _CAP:
        from conftest import make_scene
        sc = make_scene(**{**K._MASKED, "n_ants": 8, "seed": _CAP[scene]}, zero_s_slots=False)
        sc.cell.rcs = np.asarray(CAP_RCS, dtype=np.float64)
        sc.rp = O.radar_params(sc.cell, sc.carrier, sc.wave)
        return sc
    return K.make(scene) if scene in K.OWN else B.make(scene)


def is_upa(scene):
    return scene.startswith("upa")


# the cases of tests/test_beam_clean_cpu.py and tests/test_gpu_beam_clean.py: name -> (scene, beam set, keywords of ``beam_clean``)
CASES = {
    "cap8": (CAP, "b5", {}),
    "cap8_span0": (CAP, "b5", dict(span_rows=0)), "cap8_span1": (CAP, "b5", dict(span_rows=1)),
    "cap8_one": (CAP, "b5", dict(max_iter=1)),                               # the closing pass after max_iter entries, with cells left
    "cap8_tol0": (CAP, "b5", dict(merge_tol=0.0)), "cap8_bigtol": (CAP, "b5", dict(merge_tol=1e6)),
    "cap8_goca": (CAP, "b5", dict(method="GOCA")),
    "masked_gap": ("masked_gap", "b5", dict(sym_active=GAP_MASK)), "masked_gap_nomask": ("masked_gap", "b5", {}),
    "a4_24prb_generic_b37": ("a4_24prb_generic", "b37", {}),
    "a4_24prb_generic_b361": ("a4_24prb_generic", "b361", {}),
    "a4_24prb_generic_soca": ("a4_24prb_generic", "b5", dict(method="SOCA")),
    "a4_24prb_generic_allrows": ("a4_24prb_generic", "b5", dict(span_rows="nr")),   # span_rows = nr: the band is the whole window, clipped at both edges
    "a4_24prb_truncated_os": ("a4_24prb_truncated", "b5", dict(method="OS", rank=18)),
    "a6_24prb": ("a6_24prb", "b5", {}),
    "a16_24prb_b1": ("a16_24prb", "b1", {}), "a16_24prb_b16": ("a16_24prb", "b16", {}),
    "upa2x4_24prb": ("upa2x4_24prb", "b5", {}),
    # the asymmetric guard / training bands T.READER_BANDS (hr = 4, hc = 5, gr = 1, gc = 3, N = 78) on the beam planes' detector and on the rows the passes cancel on
    "bands_b5": (T.BAND_SCENE, "b5", {}), "bands_b16_goca": (T.BAND_SCENE, "b16", dict(method="GOCA")), "bands_b5_soca": (T.BAND_SCENE, "b5", dict(method="SOCA")),
    "bands_b5_os": (T.BAND_SCENE, "b5", dict(method="OS", rank=58)),
}
SCENES = tuple(dict.fromkeys(s for s, _, _ in CASES.values()))


def keywords(case, g):
    """The case's keywords with span_rows = "nr" resolved against the window."""
    kw = dict(CASES[case][2])
    if kw.get("span_rows") == "nr":
        kw["span_rows"] = g.n_rows
    return kw


@functools.lru_cache(maxsize=None)
def oracle_rows(scene):
    """Oracle only: O.mono_static_sensing -> the window's range rows and the geometry.  Computed once per scene and shared; callers must not modify it."""
    sc = make(scene)
    rp = sc.rp
    cf = T.oracle_config(scene, rp)                                        # the default bands for every scene but T.BAND_SCENE
    g = K.geometry(rp, cf)
    echo = O.mono_static_sensing(sc.tx_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, sc.noise, nfft=sc.wave.Nfft)
    rows = R.range_rows(echo, sc.tx_grid, g.n_ifft)[g.first_row - 1:g.first_row - 1 + g.n_rows].copy()
    return SimpleNamespace(sc=sc, rp=rp, cf=cf, g=g, rows=rows, L=rows.shape[1])


@functools.lru_cache(maxsize=None)
def weights(scene, beams):
    """(W [A x B], the beams' azimuth labels) of a beam set of tests/_beam_detect_restatement.py on a scene.  Shared: not to be modified."""
    return B.weights(make(scene), beams)


@functools.lru_cache(maxsize=None)
def oracle_beam_clean(case):
    """The oracle-only result of a case.  Computed once and shared; callers must not modify it."""
    scene, beams, _ = CASES[case]
    s = oracle_rows(scene)
    W, azi = weights(scene, beams)
    return beam_clean(s.rows, s.g, W, beam_azi=azi, **keywords(case, s.g))


def true_velocity(rp, q):
    return float(rp.targetRealPos[q]["Velocity"])
