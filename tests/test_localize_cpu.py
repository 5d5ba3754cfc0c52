"""Multi-static localisation without a GPU (include/isac_localize.h): the restatement of tests/_localize_restatement.py on exact scenes, the
conditioning of every scene tests/test_gpu_localize.py compares the device on, the binding's lines for the stand-alone header, and the two host helpers.
  1. noiseless measurements recover positions and velocities to rounding; in the three-node range-only scene every ghost is rejected; the two-node mirror ambiguity
     appears without azimuth and disappears with it
  2. every device scene: the map's rounding bound is <= 1e-10; the refined positions' bound, from the restatement's own H, is <= 1e-8 m; no comparison that decides an
     integer result (peak neighbours, minScore, candidate order, best measurement per link, gate, det, maxMove) is closer than 1e4 map bounds
  3. the two lines of _lib.LOCALIZE_PROTOTYPES re-derived from the header; the library exports both names and load() applied them
  4. linkMeasurements and getPositionRMSE on hand-made lists"""
from __future__ import annotations

import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import _abi_header as H
import _localize_restatement as R
from conftest import load_pkg

MAP_BOUND_MAX = 1e-10
POS_BOUND_MAX = 1e-8
DECIDABLE = 1e4                                                             # map bounds


# ---------------------------------------------------------------- 1
def _nearest(pos, truth):
    return np.array([np.hypot(*(np.asarray(truth)[:, :2] - p).T.astype(np.float64)).min() for p in pos.astype(np.float64)])


def test_noiseless_measurements_are_recovered_and_ghosts_rejected():
    sc = R.prototype_scene("three_nodes", err=None)
    ref = R.localize(sc, R.position_map(sc), **R.DEFAULTS)
    err = _nearest(ref.pos, R.TARGETS4)
    order = [int(np.hypot(*(R.TARGETS4[:, :2] - p).T.astype(np.float64)).argmin()) for p in ref.pos.astype(np.float64)]
    verr = np.abs(ref.vel.astype(np.float64) - R.VEL4[order, :2]).max()
    ghosts = int((ref.cand_status == 1).sum())
    print(f"three nodes, noiseless: position errors {err.tolist()} m, velocity error {verr:.3e} m/s, scores {ref.score.astype(float).tolist()}, rms {ref.rms.astype(float).tolist()}; "
          f"{len(ref.cand_cell)} map peaks, {ghosts} ghosts dropped")
    assert len(ref.pos) == 4 and sorted(order) == [0, 1, 2, 3] and (ref.n_links == 9).all() and (ref.vel_status == 0).all()
    assert err.max() <= 1e-9 and verr <= 1e-9 and float(ref.rms.max()) <= 1e-9
    assert ghosts >= 1 and ghosts == len(ref.cand_cell) - 4 and set(ref.cand_status.tolist()) == {0, 1}      # every other peak is a ghost, and every ghost is dropped
    for t, k in zip(ref.assoc, order):                                      # target k's measurement of every link: exact_meas lists link by link, target by target
        assert t.tolist() == [4 * link + k for link in range(9)]


def test_two_node_mirror_ambiguity_needs_azimuth():
    nodes = np.array([[0.0, 0.0, 25.0], [800.0, 0.0, 25.0]])
    targets = R.TARGETS4 * np.array([1.0, 0.8, 1.0])
    mirror = targets * np.array([1.0, -1.0, 1.0])
    links = R.all_links(2)
    grid = (0.0, 2.0, 401, -400.0, 2.0, 401)
    got = {}
    for azimuth in (False, True):
        sc = R.make_scene(nodes, links, R.exact_meas(nodes, links, targets, R.VEL4, azimuth=azimuth), grid, 1.5)
        ref = R.localize(sc, R.position_map(sc), **R.DEFAULTS)
        got[azimuth] = (_nearest(ref.pos, targets), _nearest(ref.pos, mirror))
        print(f"two nodes, azimuth {azimuth}: {len(ref.pos)} targets; distance to the truth {got[azimuth][0].tolist()}, to the mirror image {got[azimuth][1].tolist()}")
        assert len(ref.pos) == 4
    assert (np.minimum(*got[False]) <= 1e-6).all() and (got[False][1] <= 1e-6).any()       # on the truth or its image, and at least one image
    assert (got[True][0] <= 1e-6).all()


# ---------------------------------------------------------------- 2
@pytest.mark.parametrize("name", list(R.MAP_SCENES))
def test_map_scenes_have_a_small_rounding_bound(name):
    sc = R.map_scene(name)
    _, N, K, M, grid, azimuth, _ = R.MAP_SCENES[name]
    fin = ~np.isnan(sc.azi)
    print(f"{name}: bound {sc.bound:.3e}; map in [{float(sc.ref_map.min()):.3e}, {float(sc.ref_map.max()):.3e}]; {int(fin.sum())} of {M} azimuths finite")
    assert (len(sc.nodes), len(sc.links), len(sc.link)) == (N, K, M) and sc.ref_map.shape == (grid[5], grid[2])
    assert {"all": fin.all(), "none": not fin.any(), "mixed": fin.any() and not fin.all()}[azimuth]
    assert not np.array_equal(sc.order, np.arange(M)) or M <= 2              # given unsorted: the wrapper's stable sort is exercised
    assert 0 < sc.bound <= MAP_BOUND_MAX
    assert float(sc.ref_map.max()) > 0.4                                    # some link agrees somewhere: the map is not all underflow


def test_special_map_scenes_hold_what_they_are_for():
    sc = R.map_scene("g67x129_m65_k9_n64")
    m0 = int(np.flatnonzero(sc.order == 0)[0])                              # the measurement given first
    xs, ys = R.grid_xy(sc)
    X, Y = np.meshgrid(xs, ys)
    assert sc.r[m0] == 1.0e4 and float(np.exp(-R.q_of(sc, m0, X, Y).astype(np.float64) / 2).max()) == 0.0   # underflows in fp64 everywhere
    sc = R.map_scene("g67x129_m17_k9_n3")
    assert float(xs[3]) == sc.nodes[0][0] and float(ys[2]) == sc.nodes[0][1] and sc.nodes[0][2] == sc.height   # a node exactly on a grid point
    assert (sc.links == 0).any()


@pytest.mark.parametrize("name", list(R.CHAIN_SCENES))
def test_chain_scenes_are_decidable(name):
    sc = R.chain_scene(name)
    ref, mg = sc.ref, sc.ref.margins
    print(f"{name}: map bound {sc.bound:.3e}; statuses {ref.cand_status.tolist()}; {len(ref.pos)} targets, n_links {ref.n_links.tolist()}, vel_status {ref.vel_status.tolist()}; "
          f"position bounds {ref.pos_bound.tolist()} m, velocity bounds {ref.vel_bound.tolist()}, rms bounds {ref.rms_bound.tolist()}; margins {mg}")
    assert 0 < sc.bound <= MAP_BOUND_MAX
    assert (ref.pos_bound <= POS_BOUND_MAX).all() and (ref.vel_bound <= POS_BOUND_MAX).all() and (ref.rms_bound <= POS_BOUND_MAX).all()
    for kind in ("peak", "minScore", "order", "best", "gate", "det", "maxMove"):
        assert mg[kind] > DECIDABLE * sc.bound, kind
    want = {"three_nodes": {0, 1}, "two_nodes": {0}, "status_1": {1}, "status_2": {2}, "status_3": {0, 3}, "one_doppler": {0, 1}}[name]
    assert set(ref.cand_status.tolist()) >= want - {0} and (0 in want) == (len(ref.pos) > 0)
    if name in ("three_nodes", "two_nodes"):
        err = _nearest(ref.pos, R.TARGETS4)
        print(f"{name}: four of four; position errors {err.tolist()} m")
        assert len(ref.pos) == 4 and err.max() < 1.0 and (ref.vel_status == 0).all()
    if name == "one_doppler":
        assert len(ref.pos) == 4 and (ref.vel_status == 1).all() and np.isnan(ref.vel.astype(np.float64)).all()


# ---------------------------------------------------------------- 3
@pytest.fixture(scope="module")
def lib_path():
    import __graft_entry__ as g
    g.build()
    p = load_pkg().library_path()
    assert os.path.exists(p)
    return p


def test_localize_prototypes_match_the_header(lib_path):
    L = load_pkg()._lib
    header = "isac_localize.h"
    assert list(L.LOCALIZE_PROTOTYPES) == [header] and header not in H.includes() and header not in L.HEADER_PROTOTYPES and header not in L.STANDALONE_PROTOTYPES
    assert re.search(r'^#include "isac\.h"', H.text(header), flags=re.M) and "isac_localize.h" not in H.text("isac.h")
    protos = H.prototypes(header)
    table = L.LOCALIZE_PROTOTYPES[header]
    assert [(name, len(types)) for _, name, types in protos] == [("isac_position_map_dev", 22), ("isac_localize_dev", 40)]
    assert [name for _, name, _ in protos] == list(table) and not set(table) & set(L.PROTOTYPES)
    for ret, name, types in protos:
        restype, argtypes = table[name]
        assert restype is H.RETURNS[ret], name
        assert len(argtypes) == len(types), name
        for i, (got, c_type) in enumerate(zip(argtypes, types)):
            assert got is H.rule(c_type, L), f"{name} argument {i}: {c_type}"
    assert protos[1][2][:21] == protos[0][2][:21] and protos[0][2][21] == "double*" and protos[1][2][21] == "const double*"      # the same scene, the map out and in
    raw = ctypes.CDLL(lib_path)
    assert all(hasattr(raw, name) for name in table)
    lib = L.load()
    for name, (restype, argtypes) in table.items():                         # and load() applied the table
        fn = getattr(lib, name)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name
    m = re.search(r"#define ISAC_ABI_VERSION (\d+)", H.text("isac.h"))
    assert int(m.group(1)) == 8 == L.ISAC_ABI_VERSION
    for name in ("MAX_NODES", "MAX_LINKS", "MAX_MEAS", "MAX_CAND"):
        assert int(re.search(rf"#define ISAC_LOCALIZE_{name} (\d+)", H.text(header)).group(1)) == getattr(L, "ISAC_LOCALIZE_" + name)


def test_refusals_need_no_gpu(lib_path):
    """The NULL-context refusal of both calls, through the prototypes load() applied."""
    lib = load_pkg()._lib.load()
    scene = (None, None, 1, None, None, 1, *([None] * 7), 1, 0.0, 1.0, 1, 0.0, 1.0, 1, 0.0, None)
    assert lib.isac_position_map_dev(*scene) == 1
    assert lib.isac_localize_dev(*scene, 0.5, 1, 1, 4.0, 1, 1.0, 1, *([None] * 11)) == 1


# ---------------------------------------------------------------- 4
def test_link_measurements_from_hand_made_lists():
    pkg = load_pkg()
    rp = SimpleNamespace(rRes=9.75, vRes=1.25)
    lists = [dict(rng=np.array([100.0, 150.0]), vel=np.array([3.0, -4.0]), azi=np.array([10.0, -20.0])),
             dict(rng=np.array([], dtype=np.float64), vel=np.array([], dtype=np.float64), azi=np.array([], dtype=np.float64)),
             dict(rng=np.array([120.0, 121.0, 200.0]), vel=np.array([1.0, 1.5, 2.0]), azi=np.array([5.0, 6.0, 7.0]), sidelobe_of=np.array([-1, 0, -1]), nu=np.zeros(3))]
    links = [(0, 0), (0, 1), (1, 0)]
    m = pkg.sensing.estimation.linkMeasurements(lists, links, rp)
    assert m["link"].tolist() == [0, 0, 2, 2] and m["index"].tolist() == [0, 1, 0, 2] and m["link"].dtype == np.int32
    assert m["r"].tolist() == [200.0, 300.0, 240.0, 400.0] and m["s"].tolist() == [6.0, -8.0, 2.0, 4.0] and m["azi"].tolist() == [10.0, -20.0, 5.0, 7.0]
    assert (m["sigma_r"] == 9.75).all() and (m["sigma_v"] == 1.25).all() and (m["sigma_a"] == 2.0).all()
    m = pkg.sensing.estimation.linkMeasurements(lists, links, rp, sigmaRange=3.0, sigmaVel=0.5, sigmaAzi=1.0, useAzimuth=False)
    assert np.isnan(m["azi"]).all() and (m["sigma_r"] == 3.0).all() and (m["sigma_v"] == 0.5).all() and (m["sigma_a"] == 1.0).all() and m["r"].size == 4
    with pytest.raises(ValueError):
        pkg.sensing.estimation.linkMeasurements(lists[:2], links, rp)
    with pytest.raises(ValueError):
        pkg.sensing.estimation.linkMeasurements([dict(rng=[1.0], vel=[], azi=[1.0])], links[:1], rp)


def test_position_rmse_on_hand_made_positions():
    f = load_pkg().sensing.postProcessing.getPositionRMSE
    truth = np.array([[0.0, 0.0, 1.5], [10.0, 0.0, 1.5], [100.0, 100.0, 1.5]])
    est = dict(pos=np.array([[3.0, 4.0], [1.0, 0.0], [9.0, 0.0], [100.0, 104.0], [100.0, 100.5]]))
    r = f(est, truth, 6.0)
    # the first takes truth 0 (5 m); the second finds truth 0 gone and truth 1 at 9 m, outside the gate; the third takes truth 1; the fourth truth 2; the fifth finds it gone
    assert r.match.tolist() == [0, -1, 1, 2, -1]
    assert r.posRMSE[[0, 2, 3]].tolist() == [5.0, 1.0, 4.0] and np.isnan(r.posRMSE[[1, 4]]).all()
    assert f(est, truth, 5.0).match.tolist() == [-1, 0, 1, 2, -1]           # the gate is strict, as getRMSE's
    assert f(np.array([[10.0, 1.0]]), truth[:, :2], 2.0).posRMSE.tolist() == [1.0]
    r = f(dict(pos=np.zeros((0, 2))), truth, 1.0)
    assert isinstance(r, float) and np.isnan(r)
