"""Beamformed detection (isac_fft2d_get_rdm_window / isac_fft2d_beam_detect; project-defined, include/isac_beams.h) without a GPU: the conditioning of every case
tests/test_gpu_beam_detect.py runs, the matched gain of the two-way weight, the weak-target scene that motivates the call, the restatement's own rules, the host-side
beamWeights and the binding's prototype lines.  The device library is not asked for anything but its symbol table."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_pkg

import _abi_header as H
import _beam_detect_restatement as R


@pytest.mark.parametrize("case", R.CASES, ids=["-".join(map(str, c)) for c in R.CASES])
def test_case_conditioning(case):
    """Oracle stages -> restatement for every case of the GPU tests: at least one target, and EVERY margin of every decision -- each CUT of each beam against its
    threshold, each target against its strongest neighbour, each detected near-miss, each b* against the best different beam value -- at least 1e-9: the GPU tests then
    leave out and skip nothing."""
    t = R.oracle_beam_detect(*case)
    print(f"{case}: {t.row.size} targets, {int(t.offsets[-1])} detections; rows {t.row[:6].tolist()} cols {t.col[:6].tolist()} beam {t.beam[:6].tolist()} "
          f"hits {t.hits[:6].tolist()}; margins: detection {t.margin_det:.3e}, near miss {t.near_miss:.3e}, local maximum {t.margin_max.min():.3e}, beam {t.margin_beam.min():.3e}")
    assert t.row.size >= 1
    assert (R.margins(t) >= R.GUARD_BAND).all()
    assert all((r > 1.0).all() for r in t.det_ratio)


@pytest.mark.parametrize("name,n_ants", [("a16_24prb", 16), ("a4_24prb_generic", 4)])
def test_matched_gain_of_the_two_way_weight(name, n_ants):
    """At the strongest cell of a 24-PRB scene, |w' x|^2 / (w' w) over the antenna-mean power: A (within 1 %) for w = s .* s, s the receive steering vector of the
    target there; below 1.6 for s, conj(s) and conj(s .* s)."""
    sc, w = R.make(name), R.oracle_window(name)
    S = (np.abs(w.win) ** 2).sum(axis=2)
    i, j = np.unravel_index(np.argmax(S), S.shape)
    x = w.win[i, j, :]
    mean_p = S[i, j] / n_ants
    gains = {}
    for q in range(sc.rp.RxSteeringVec.shape[1]):
        s = sc.rp.RxSteeringVec[:, q]
        for label, wt in (("s.*s", s * s), ("s", s), ("conj(s)", np.conj(s)), ("conj(s.*s)", np.conj(s * s))):
            gains[(q, label)] = abs(np.vdot(wt, x)) ** 2 / np.vdot(wt, wt).real / mean_p
    q = max(range(sc.rp.RxSteeringVec.shape[1]), key=lambda k: gains[(k, "s.*s")])
    print(f"{name}: strongest cell ({i + w.first_row}, {j + w.first_col}), target {q + 1}: " + ", ".join(f"{l} {gains[(q, l)]:.3f}" for l in ("s.*s", "s", "conj(s)", "conj(s.*s)")))
    assert abs(gains[(q, "s.*s")] - n_ants) <= 0.01 * n_ants
    assert all(gains[(q, l)] < 1.6 for l in ("s", "conj(s)", "conj(s.*s)"))


def test_weak_target_is_seen_by_the_beam_and_by_no_antenna():
    """a8_273prb with the second target's echo amplitude x 0.1: no antenna's CA-CFAR list holds its cell (152, 124) and fft2D's rngEst has no 184.2 m; the plane
    beamformed with the matched two-way weight detects it.  The ratios are printed, not asserted beyond the 1e-9 band."""
    import _cfar_methods_restatement as C
    sc, w = R.make(R.WEAK), R.oracle_window(R.WEAK)
    cell = (152, 124)
    assert abs(sc.rp.largeScaleFading[1] / R.make("a8_273prb").rp.largeScaleFading[1] - 0.1) < 1e-12
    holds = [bool(((d[0] == cell[0]) & (d[1] == cell[1])).any()) for d in w.detections]
    rng_cell = (cell[0] - 1) * sc.rp.rRes
    assert abs(rng_cell - 184.2) < 0.05
    assert sum(holds) == 0 and len(holds) == 8
    assert not np.any(np.abs(w.rng_est - rng_cell) < 0.5 * sc.rp.rRes)
    alpha = C.threshold_factor("CA", C.n_train(R.GUARD, R.TRAIN), float(sc.rp.Pfa))
    local = np.array([[cell[0] - w.first_row + 1], [cell[1] - w.first_col + 1]])
    ratios = []
    for a in range(8):
        P = np.abs(w.win[:, :, a]) ** 2
        _, thr = C.detect(P, local, R.GUARD, R.TRAIN, "CA", alpha, return_threshold=True)
        ratios.append(float(P[local[0, 0] - 1, local[1, 0] - 1] / thr[0]))
    t = R.oracle_beam_detect(R.WEAK, "b1_t2", "CA", 1)
    k = np.flatnonzero((t.detections[0][0] == cell[0]) & (t.detections[0][1] == cell[1]))
    print(f"per-antenna P / thr at {cell}: largest {max(ratios):.3f}, smallest {min(ratios):.3f}; beam P / thr {t.det_ratio[0][k].tolist()}; "
          f"beam detections {int(t.offsets[-1])}; per-antenna detections {[d.shape[1] for d in w.detections]}")
    assert all(abs(r - 1.0) >= R.GUARD_BAND for r in ratios) and max(ratios) < 1.0
    assert k.size == 1 and t.det_ratio[0][k[0]] - 1.0 >= R.GUARD_BAND
    i = np.flatnonzero((t.row == cell[0]) & (t.col == cell[1]))
    assert i.size == 1 and t.beam[i[0]] == 1 and t.hits[i[0]] == 1


def test_restatement_rules():
    """max_map: first arg-max in ascending plane order, a NaN never wins, NaN only where every plane is; beam_planes against a direct evaluation; a plateau gives no
    target."""
    nan = np.nan
    P = np.array([[[1.0, 3.0, 3.0], [nan, 2.0, 1.0]], [[nan, nan, nan], [5.0, nan, 5.0]]])
    M, arg = R.max_map(P)
    assert np.array_equal(M, np.array([[3.0, 2.0], [nan, 5.0]]), equal_nan=True) and np.array_equal(arg, [[1, 1], [0, 0]])
    rng = np.random.default_rng(3)
    Y = rng.standard_normal((5, 4, 3)) + 1j * rng.standard_normal((5, 4, 3))
    W = rng.standard_normal((3, 2)) + 1j * rng.standard_normal((3, 2))
    want = np.abs(np.einsum("ab,rca->rcb", W.conj(), Y)) ** 2 / (np.abs(W) ** 2).sum(axis=0)
    assert np.allclose(R.beam_planes(Y, W), want, rtol=1e-13, atol=0)
    P = np.ones((5, 5, 1))
    P[2, 2, 0] = P[2, 3, 0] = 2.0                                             # two equal neighbours: a plateau
    det = [np.array([[3, 3], [3, 4]])]
    t = R.beam_cells(P, det, 1, 1, (2, 4, 2, 4), 8)
    assert t.row.size == 0
    P[2, 2, 0] = 2.5
    t = R.beam_cells(P, det, 1, 1, (2, 4, 2, 4), 8)
    assert t.row.tolist() == [3] and t.col.tolist() == [3] and t.hits.tolist() == [1] and t.beam.tolist() == [1] and t.margin_beam.tolist() == [1.0]


def test_beam_weights_are_the_squared_steering_vectors_of_radar_params():
    """beamWeights(rp, azimuth, elevation) at the targets' own directions = RxSteeringVec .* RxSteeringVec bit for bit, for a ULA and a UPA, on the oracle's radarParams
    and on the product's (one steering expression, factored out of radarParams)."""
    pkg = load_pkg()
    for name in ("a6_24prb", "upa2x4_24prb"):
        sc = R.make(name)
        dirs = [R.target_direction(sc, q) for q in range(2)]
        azi, ele = [d[0] for d in dirs], [d[1] for d in dirs]
        for rp in (sc.rp, pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)):
            W = pkg.sensing.estimation.beamWeights(rp, azi, ele)
            assert W.shape == (sc.A, 2) and W.tobytes(order="F") == np.asfortranarray(rp.RxSteeringVec * rp.RxSteeringVec).tobytes(order="F")
        assert np.array_equal(pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave).RxSteeringVec, sc.rp.RxSteeringVec)
    sc = R.make("a6_24prb")
    assert np.array_equal(pkg.sensing.estimation.beamWeights(sc.rp, 20.0), pkg.sensing.estimation.beamWeights(sc.rp, [20.0], [0.0]))
    with pytest.raises(ValueError):
        pkg.sensing.estimation.beamWeights(sc.rp, [1.0, 2.0], [0.0])


def test_binding_has_the_prototypes_and_the_abi_is_unchanged():
    """include/isac_beams.h is additive under ABI 8: no new struct, no new isac_abi_sizeof selector; isac_fft2d_get_rdm_window takes the arguments of
    isac_fft2d_get_power_window, and both functions refuse a NULL context.  (Their prototype lines are compared with the header by tests/test_abi_cpu.py, row
    "isac_beams.h".)"""
    import __graft_entry__ as g
    g.build()
    L = load_pkg()._lib
    hdr = open(os.path.join(ROOT, "include", "isac_beams.h")).read()
    plain = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    assert "typedef" not in plain and "ISAC_SIZEOF" not in plain
    assert int(re.search(r"#define ISAC_MAX_BEAMS (\d+)", plain).group(1)) == L.ISAC_MAX_BEAMS
    lib = L.load()                                                             # (needs no GPU)
    a = {name: params for _, name, params in H.declarations("isac.h")}["isac_fft2d_get_power_window"]
    b = {name: params for _, name, params in H.declarations("isac_beams.h")}["isac_fft2d_get_rdm_window"]
    assert a.replace("double* P", "isac_c64* Y") == b                          # arguments exactly as isac_fft2d_get_power_window, with isac_c64 for double
    assert lib.isac_abi_version() == 8 == L.ISAC_ABI_VERSION and lib.isac_abi_sizeof(13) == -1
    assert lib.isac_fft2d_get_rdm_window(None, None, 0, None, None, None) == 1   # refused before anything touches a device: no context (ISAC_ERR_INVALID_ARG)
    assert lib.isac_fft2d_beam_detect(None, None, 0, None, None, None, None, None, None, 0, None, None, None) == 1
    est = load_pkg().sensing.estimation
    assert callable(est.rdmWindow) and callable(est.beamWeights) and callable(est.beamDetect)
