"""Multi-static echo synthesis (project-defined, include/isac_multistatic.h) without a GPU: the restatement against the oracle, the geometry helper against radarParams and
against the formulas, the header and the binding's prototype lines, and the conditioning of the three physical scenes tests/test_gpu_multistatic.py runs on the device.  The
device library is not asked for anything but its symbol table."""
from __future__ import annotations

import copy
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import oracle as O
import _multistatic_restatement as M
import _numerology_scenes as N
from conftest import ROOT, load_pkg
from test_gpu_numerology import MARGIN                                     # the bound the numerology scenes are held to: 1e-6

RR_TARGET_SAMPLES, BISTATIC_SAMPLES = 33, 44                               # the own echo's and the bistatic path's delay in samples (x rRes: 161.02 m and 214.695 m)


@pytest.fixture(scope="module")
def binding():
    import __graft_entry__ as g
    g.build()
    return load_pkg()._lib


# ---------------------------------------------------------------- (a) the restatement is the oracle on mono-static paths
@pytest.mark.parametrize("targets,velocity,los", [(N.NEAR1, (5.0,), (1,)), (N.PAIR, (10.0, -6.0), (1, 1)), (N.PAIR + N.SMALL, (10.0, -6.0, 3.0), (1, 0, 1))],
                         ids=["q1", "q2", "q3_one_nlos"])
def test_restatement_with_mono_static_paths_is_the_oracle(targets, velocity, los):
    sc = N.scene(60, 11, 3, 1, targets, velocity, 6, False, seed=5)
    los = np.asarray(los, dtype=np.uint8)
    p = M.mono_static_paths(sc.rp, los)
    assert len(p.source) == int(los.sum())
    for noise in (None, sc.noise):
        want = O.basic_radar_channel(sc.tx_wave, sc.rp, los, noise)
        got = M.multi_static_channel([sc.tx_wave], sc.rp.fc, sc.rp.fs, sc.rp.N0, sc.A, M.path_tuples(p), noise)
        assert got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(M.multi_static_sensing([sc.tx_wave], sc.L + 2, sc.K, sc.wave.Nfft, 60, sc.rp.fc, sc.rp.fs, sc.rp.N0, sc.A, M.path_tuples(p), sc.noise),
                          O.mono_static_sensing(sc.tx_wave, (sc.K, sc.L + 2, sc.A), sc.carrier, sc.rp, los, sc.noise, nfft=sc.wave.Nfft))
    with pytest.raises(ValueError):
        M.multi_static_channel([sc.tx_wave], sc.rp.fc, sc.rp.fs, sc.rp.N0, sc.A, [], None)


# ---------------------------------------------------------------- (b) the geometry helper
def _targets_of(cell, vel_vectors):
    return [SimpleNamespace(position=np.asarray(cell.targetPosition[k], dtype=np.float64), velocity=np.asarray(vel_vectors[k], dtype=np.float64), rcs=float(cell.rcs[k]))
            for k in range(int(cell.numTargets))]


def test_paths_of_the_own_cell_are_radar_params_exactly():
    """j = i: largeScaleFading, RxSteeringVec, ceil(2 R / c / Ts) and 2 v / lambda of sensing.radarParams on the same targets, to the bit; a blocked target is left out."""
    pkg = load_pkg()
    sc = N.scene(60, 24, 4, 1, N.PAIR + N.SMALL, (0.0, 0.0, 0.0), 6, False, seed=3, with_noise=False)
    vel = [np.array([3.0, -4.0, 0.5]), np.array([-7.0, 2.0, 0.0]), np.array([0.0, 11.0, 0.0])]
    cell = copy.copy(sc.cell)
    cell.velocity = np.array([-(vel[k] @ (cell.targetPosition[k] - cell.gNBPosition)) / np.linalg.norm(cell.targetPosition[k] - cell.gNBPosition) for k in range(3)])
    rp = pkg.sensing.radarParams(cell, sc.carrier, sc.wave)
    p = pkg.sensing.channelModels.multiStaticPaths(cell, [cell], _targets_of(cell, vel), carrierInfo=sc.carrier, waveInfo=sc.wave, targetLoS=[[1, 0, 1]])
    keep = [0, 2]
    lam = O.LIGHTSPEED / rp.fc
    assert p.kind == [("target", 0, 0), ("target", 0, 2)] and p.source.tolist() == [0, 0]
    assert np.array_equal(p.gain, rp.largeScaleFading[keep]) and np.array_equal(p.rxSteering, rp.RxSteeringVec[:, keep])
    assert all(np.array_equal(p.txSteering[i], rp.RxSteeringVec[:, k]) for i, k in enumerate(keep))
    assert np.array_equal(p.shift, np.asarray(N.delays_of(rp))[keep]) and np.array_equal(p.doppler, (2.0 * rp.velocity / lam)[keep])
    assert p.doppler[0] != 0 and p.shift.dtype == np.int64 and p.source.dtype == np.int32
    q = M.mono_static_paths(O.radar_params(cell, sc.carrier, sc.wave), [1, 0, 1])                # ... and the oracle's record gives the same list
    assert np.array_equal(p.shift, q.shift) and np.array_equal(p.doppler, q.doppler) and np.array_equal(p.gain, q.gain) and np.array_equal(p.rxSteering, q.rxSteering)


def test_bistatic_and_direct_paths_follow_their_formulas():
    """Against the formulas restated in tests/_multistatic_restatement.py (1e-13 relative: two ways of rounding the same expression); the bistatic gain, delay and Doppler are
    symmetric in j <-> i to the bit; LoS flags and the wall loss do what they say."""
    pkg = load_pkg()
    b = M.base()
    sc = b.sc
    lam, ts = O.LIGHTSPEED / sc.rp.fc, 1.0 / sc.rp.fs
    tg = [SimpleNamespace(position=np.array([150.0, 40.0, 1.5]), velocity=np.array([6.0, -3.0, 0.0]), rcs=2.5)]
    kw = dict(carrierInfo=sc.carrier, waveInfo=sc.wave)
    paths = pkg.sensing.channelModels.multiStaticPaths
    p = paths(sc.cell, [sc.cell, b.nb.cell], tg, directLossdB=40.0, **kw)
    assert p.kind == [("target", 0, 0), ("direct", 1), ("target", 1, 0)] and p.source.tolist() == [0, 1, 1]
    for i, want in ((1, M.direct_path(b.nb.cell, sc.cell, lam, ts, 40.0)), (2, M.bistatic_path(b.nb.cell, sc.cell, lam, ts, tg[0].position, tg[0].velocity, tg[0].rcs))):
        assert int(p.shift[i]) == want[0] and abs(p.doppler[i] - want[1]) <= 1e-13 * max(abs(want[1]), 1.0) and abs(p.gain[i] - want[2]) <= 1e-13 * want[2]
        assert N.rel(p.txSteering[i], want[3]) <= 1e-13 and N.rel(p.rxSteering[:, i], want[4]) <= 1e-13
    assert p.doppler[1] == 0.0 and p.doppler[2] != 0.0
    free = paths(sc.cell, [sc.cell, b.nb.cell], tg, **kw)
    assert abs(free.gain[1] / p.gain[1] - 100.0) <= 1e-12 and np.array_equal(free.gain[[0, 2]], p.gain[[0, 2]])
    back = paths(b.nb.cell, [b.nb.cell, sc.cell], tg, **kw)                                    # the same pair of nodes, roles exchanged
    assert back.gain[2] == p.gain[2] and back.shift[2] == p.shift[2] and back.doppler[2] == p.doppler[2]
    assert np.array_equal(back.txSteering[2], p.rxSteering[:, 2]) and np.array_equal(back.rxSteering[:, 2], p.txSteering[2])
    assert back.gain[1] == free.gain[1] and back.shift[1] == free.shift[1]
    blocked = paths(sc.cell, [sc.cell, b.nb.cell], tg, directLoS=[1, 0], targetLoS=[[1], [0]], **kw)
    assert blocked.kind == [("target", 0, 0)]
    no_rx = paths(sc.cell, [sc.cell, b.nb.cell], tg, targetLoS=[[0], [1]], **kw)               # the receiver does not see the target: no echo of it from anyone
    assert no_rx.kind == [("direct", 1)]
    away = paths(sc.cell, [b.nb.cell], tg, targetLoS=[[1], [1]], **kw)                         # the receiver is not among the sources: its row comes last
    assert away.kind == [("direct", 0), ("target", 0, 0)] and away.gain[1] == p.gain[2]
    with pytest.raises(ValueError):
        paths(sc.cell, [b.nb.cell], tg, targetLoS=[[1]], **kw)


# ---------------------------------------------------------------- (c) header and binding
def test_binding_has_the_prototypes_and_the_abi_is_unchanged(binding):
    """include/isac_multistatic.h is additive under ABI 8: no new struct, no new isac_abi_sizeof selector; the header states the limits, the refusals and what is out of
    scope, and its two functions refuse a NULL context.  (Their prototype lines are compared with the header by tests/test_abi_cpu.py, row "isac_multistatic.h".)"""
    L = binding
    hdr = open(os.path.join(ROOT, "include", "isac_multistatic.h")).read()
    plain = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    assert "typedef" not in plain and "struct" not in plain and "ISAC_SIZEOF" not in plain
    for macro, want in (("PATHS", 64), ("SOURCES", 32), ("ANTS", 256)):
        assert int(re.search(rf"#define ISAC_MULTISTATIC_MAX_{macro} (\d+)", plain).group(1)) == want == getattr(L, f"ISAC_MULTISTATIC_MAX_{macro}")
    for word in ("OUT OF SCOPE", "MEX", "LIMITS", "n_paths 1 .. 64", "n_sources 1 .. 32", "1 .. 256", "shift >= T contributes nothing", "never read", "ISAC_ERR_NO_LOS",
                 "ISAC_ERR_INVALID_ARG", "ISAC_ERR_CAPACITY", "a refused call launches nothing and writes nothing", "bit for bit", "the same seed gives the noise bits",
                 "cached range rows and lazy echo grid"):
        assert word in hdr, word
    lib = L.load()                                                             # (needs no GPU)
    assert lib.isac_abi_version() == 8 == L.ISAC_ABI_VERSION and lib.isac_abi_sizeof(13) == -1
    assert lib.isac_multi_static_channel_dev(*([None] * 3), 1, 1, 1.0, 1.0, 0.0, 1, 1, *([None] * 6), 0, None, 0, None) == 1      # refused before anything touches a device: no context
    assert lib.isac_multi_static_sensing_dev(*([None] * 3), 1, 1, 1.0, 1.0, 0.0, 1, 1, *([None] * 6), 0, None, 0, 1, None, None, None) == 1
    pkg = load_pkg()
    assert callable(pkg.sensing.multiStaticSensing) and callable(pkg.sensing.channelModels.multiStaticChannel) and callable(pkg.sensing.channelModels.multiStaticPaths)


# ---------------------------------------------------------------- (d) the three physical scenes: restatement -> ofdm_demodulate -> fft2d / ca_cfar2d
def _check_margins(s, name):
    for what, (_, _, margin) in (("own grid", s.own), ("neighbour's grid", s.nbr)):
        print(f"{name}, {what}: guard margins {['%.3g' % m for m in margin]}")
        assert all(m > MARGIN for m in margin), f"{name}, {what}: a CUT cell lies within {min(margin):.2e} of its threshold"


def test_scene_paths_are_the_helpers():
    """The scenes' restated path lists against sensing.channelModels.multiStaticPaths on the same geometry: same paths in the same order, shifts equal, the rest to 1e-13."""
    pkg = load_pkg()
    b = M.base()
    for name, kw in M.SCENES.items():
        p = pkg.sensing.channelModels.multiStaticPaths(b.sc.cell, [b.sc.cell, b.nb.cell], b.targets, carrierInfo=b.sc.carrier, waveInfo=b.sc.wave,
                                                       directLoS=[1, kw["direct_los"]], directLossdB=kw["loss_db"])
        rows = M.restated_paths(name)
        assert len(rows) == len(p.source) == (3 if kw["direct_los"] else 2)
        for i, (s, d, f, g, tb, ra) in enumerate(rows):
            assert s == p.source[i] and d == p.shift[i] and abs(f - p.doppler[i]) <= 1e-13 and abs(g - p.gain[i]) <= 1e-13 * g
            assert N.rel(p.txSteering[i], tb) <= 1e-13 and N.rel(p.rxSteering[:, i], ra) <= 1e-13
    rows = M.restated_paths("interference")
    print(f"gains: own echo {rows[0][3]:.3e}, direct path {rows[1][3]:.3e}, bistatic echo {rows[2][3]:.3e}; shifts {[r[1] for r in rows]}")
    assert rows[0][1] == RR_TARGET_SAMPLES and rows[2][1] == BISTATIC_SAMPLES
    assert 5.7e-3 < rows[1][3] < 5.9e-3 and 2.6e-5 < rows[0][3] < 2.8e-5          # the direct path's amplitude gain, 5.8e-3, against the echo's 2.7e-5


def test_bistatic_delay_is_listed_with_the_neighbours_grid_only():
    s, sc = M.scene("bistatic"), M.base().sc
    _check_margins(s, "bistatic")
    r_res = sc.rp.rRes
    (est_own, dets_own, _), (est_nbr, dets_nbr, _) = s.own, s.nbr
    print(f"bistatic: rngEst with the own grid {est_own.rngEst.tolist()}, with the neighbour's {est_nbr.rngEst.tolist()}")
    assert est_nbr.rngEst[0] == BISTATIC_SAMPLES * r_res and abs(BISTATIC_SAMPLES * r_res - 214.695) < 1e-3
    assert BISTATIC_SAMPLES * r_res not in est_own.rngEst.tolist() and est_own.rngEst[0] == RR_TARGET_SAMPLES * r_res and abs(RR_TARGET_SAMPLES * r_res - 161.02) < 1e-2
    assert RR_TARGET_SAMPLES * r_res not in est_nbr.rngEst.tolist()
    alone = N.oracle_of(N.CASE[M.SCENE_CASE])                                  # the list with the own grid is the list of the cell alone
    assert np.array_equal(est_own.rngEst, alone.est.rngEst) and all(np.array_equal(a, b) for a, b in zip(dets_own, alone.dbg.detections))


def test_direct_path_of_the_neighbour_blinds_the_cell():
    s = M.scene("interference")
    _check_margins(s, "interference")
    est_own, dets_own, _ = s.own
    alone = N.oracle_of(N.CASE[M.SCENE_CASE])
    assert all(d.shape[1] == 3 for d in alone.dbg.detections)                  # the target came with three detections per antenna
    assert est_own is None and all(d.shape[1] == 0 for d in dets_own)          # ... and is gone: findpeaks raises on the empty list


def test_a_wall_in_the_direct_path_brings_the_detections_back():
    s = M.scene("wall")
    _check_margins(s, "wall")
    est_own, dets_own, _ = s.own
    alone = N.oracle_of(N.CASE[M.SCENE_CASE])
    assert est_own is not None and all(np.array_equal(a, b) for a, b in zip(dets_own, alone.dbg.detections)) and np.array_equal(est_own.rngEst, alone.est.rngEst)
