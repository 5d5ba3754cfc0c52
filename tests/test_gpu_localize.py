"""Multi-static localisation on the MI355X (project-defined -- include/isac_localize.h): isac_position_map_dev and isac_localize_dev
(csrc/localize.hip) against tests/_localize_restatement.py.  tests/test_localize_cpu.py has shown without a GPU that every scene's map bound is below 1e-10, every
position bound below 1e-8 m, and that no comparison deciding an integer result is closer than 1e4 map bounds.
  1. the map against the restatement within the scene's bound: every grid, M, K, N and azimuth mix; two calls give the same bits
  2. hand-made maps: plateau, equal peaks, edge and corner peaks, truncation by maxCand and maxTargets, nothing above minScore
  3. the full chain on the prototype scenes; statuses 1 to 3 and the NaN velocity
  4. refusals leave poisoned outputs untouched
  5. the context's last CPI, its getters' answers and a pending submit are the same bytes before and after
  6. end to end: two cells, four links through multiStaticSensing -> fft2D -> targetList -> refineTargets -> refineRange -> linkMeasurements -> localizeTargets"""
from __future__ import annotations

import ctypes as C
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest

import _localize_restatement as R

pytestmark = pytest.mark.gpu

POISON = -7.25e300
IPOISON = -7


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context()
    yield c
    c.close()


def _mod(pkg):
    return import_module(pkg.__name__ + ".sensing.estimation.localizeTargets")


def _scene(pkg, sc):
    return _mod(pkg).Scene(sc.nodes, sc.links, sc.given, sc.grid, sc.height)


def _device_map(pkg, ctx, sc):
    d = _mod(pkg).position_map(ctx, _scene(pkg, sc))
    try:
        return np.ascontiguousarray(d.numpy().T)                            # [ny x nx]
    finally:
        d.free()


# ---------------------------------------------------------------- 1
@pytest.mark.parametrize("name", list(R.MAP_SCENES))
def test_map_against_the_restatement(pkg, ctx, name):
    sc = R.map_scene(name)
    got = _device_map(pkg, ctx, sc)
    err = float(np.abs(got.astype(R.LD) - sc.ref_map).max())
    print(f"{name}: map error {err:.3e}, bound {sc.bound:.3e} ({err / sc.bound:.3f} of it); map in [{got.min():.3e}, {got.max():.3e}]")
    assert got.shape == sc.ref_map.shape and np.isfinite(got).all()
    assert err <= sc.bound
    assert got.tobytes() == _device_map(pkg, ctx, sc).tobytes()             # two calls, the same bits


@pytest.mark.parametrize("name", ["three_nodes", "two_nodes"])
def test_prototype_maps_against_the_restatement(pkg, ctx, name):
    sc = R.chain_scene(name)
    got = _device_map(pkg, ctx, sc)
    err = float(np.abs(got.astype(R.LD) - sc.ref_map).max())
    print(f"{name}: 401 x 401 map error {err:.3e}, bound {sc.bound:.3e} ({err / sc.bound:.3f} of it)")
    assert err <= sc.bound


# ---------------------------------------------------------------- 2
def _hand_scene(nx, ny):
    """The noiseless three-node measurements over a small grid around the first target: the candidates of a hand-made map are judged on real measurements."""
    sc = R.prototype_scene("three_nodes", err=None, grid=(204.0, 2.0, nx, 304.0, 2.0, ny))
    return sc


def _run_on_map(pkg, ctx, sc, hand, fill=(0.0, 0), **par):
    """isac_localize_dev on the hand-made map [ny x nx]: (status, raw outputs) and the restatement's answer on the same map."""
    p = {**R.DEFAULTS, **par}
    scene = _scene(pkg, sc)
    dx, dy = sc.grid[1], sc.grid[4]
    min_score = p["minLinks"] - 0.5 if p["minScore"] is None else p["minScore"]
    max_move = 4.0 * float(np.hypot(dx, dy)) if p["maxMove"] is None else p["maxMove"]
    d_map = ctx.to_device(np.asfortranarray(np.asarray(hand, dtype=np.float64).T))
    try:
        st, o = _mod(pkg).localize_raw(ctx, scene, d_map, min_score, p["maxCand"], p["minLinks"], p["gate"], p["iters"], max_move, p["maxTargets"], fill=fill)
    finally:
        d_map.free()
    return st, o, R.localize(sc, np.asarray(hand, dtype=np.float64), **p)


def _same_integers(o, ref, order):
    n, nc = int(o["n_out"][0]), int(o["n_out"][1])
    assert (n, nc) == (len(ref.pos), len(ref.cand_cell))
    assert o["cand_cell"][:nc].tolist() == ref.cand_cell.tolist() and o["cand_status"][:nc].tolist() == ref.cand_status.tolist()
    assert np.array_equal(o["cand_score"][:nc], ref.cand_score.astype(np.float64))
    assert o["n_links"][:n].tolist() == ref.n_links.tolist() and o["vel_status"][:n].tolist() == ref.vel_status.tolist()
    a = o["assoc"][:n].copy()
    a[a >= 0] = order[a[a >= 0]]
    assert a.tolist() == ref.assoc.tolist()
    return n, nc


HAND_MAPS = {}


def _hand(name):
    def add(f):
        HAND_MAPS[name] = f
        return f
    return add


@_hand("plateau")
def _plateau():                                                             # equal values everywhere: exactly one candidate, the lowest index
    return np.full((5, 7), 3.0), dict(minScore=2.5), [0]


@_hand("plateau_inside")
def _plateau_inside():                                                      # a 2 x 3 plateau off the border: its lowest index
    m = np.zeros((5, 7))
    m[2:4, 3:6] = 4.0
    return m, dict(minScore=2.5), [2 * 7 + 3]


@_hand("two_equal_peaks")
def _two_equal():                                                           # index order
    m = np.zeros((5, 7))
    m[3, 5] = m[1, 1] = 5.0
    m[1, 4] = 6.0
    return m, dict(minScore=2.5), [1 * 7 + 4, 1 * 7 + 1, 3 * 7 + 5]


@_hand("edges_and_corners")
def _edges():
    m = np.zeros((5, 7))
    m[0, 0], m[0, 6], m[4, 0], m[4, 6], m[0, 3], m[2, 6], m[4, 2], m[2, 0] = 9.0, 8.0, 7.0, 6.0, 5.5, 5.0, 4.5, 4.0
    return m, dict(minScore=2.5), [0, 6, 28, 34, 3, 20, 30, 14]


@_hand("max_cand")
def _max_cand():                                                            # six peaks, three kept: the best three
    m = np.zeros((5, 7))
    for v, (iy, ix) in enumerate([(0, 0), (0, 2), (0, 4), (2, 1), (2, 3), (4, 6)]):
        m[iy, ix] = 3.0 + v
    return m, dict(minScore=2.5, maxCand=3), [34, 17, 15]


@_hand("six_blocks")
def _six_blocks():                                                          # 33 x 40 = 1320 cells: six blocks of the peak kernel; 340 peaks, 339 of them equal, 256 kept
    m = np.zeros((40, 33))
    m[0::2, 0::2] = 3.0
    m[38, 32] = 7.0
    return m, dict(minScore=2.5, maxCand=256, minLinks=10), None


@pytest.mark.parametrize("name", list(HAND_MAPS))
def test_hand_made_maps(pkg, ctx, name):
    hand, par, cells = HAND_MAPS[name]()
    sc = _hand_scene(hand.shape[1], hand.shape[0])
    st, o, ref = _run_on_map(pkg, ctx, sc, hand, **par)
    assert st == 0
    n, nc = _same_integers(o, ref, sc.order)
    print(f"{name}: candidates {o['cand_cell'][:nc].tolist()[:12]}, statuses {o['cand_status'][:nc].tolist()[:12]}, {n} targets")
    if cells is not None:
        assert ref.cand_cell.tolist() == cells
    else:
        assert nc == 256 and ref.cand_cell[0] == 38 * 33 + 32 and ref.cand_cell[1:].tolist() == sorted(ref.cand_cell[1:].tolist())


def test_max_targets_truncates_with_status_4(pkg, ctx):
    sc = R.chain_scene("three_nodes")
    got = _device_map(pkg, ctx, sc)
    st, o, ref = _run_on_map(pkg, ctx, sc, got, fill=(POISON, IPOISON), maxTargets=2)
    assert st == 0
    n, nc = _same_integers(o, ref, sc.order)
    print(f"maxTargets 2: statuses {o['cand_status'][:nc].tolist()[:8]}")
    assert n == 2 and o["cand_status"][:4].tolist() == [0, 0, 4, 4] and 0 not in o["cand_status"][4:nc].tolist()     # (unclaimed measurements of the two targets left out make further fixes: 3 and 4 occur)
    full = sc.ref                                                           # the first two of the untruncated run; the later ones claim nothing
    assert np.abs(o["pos"][:2] - full.pos[:2].astype(np.float64)).max() <= full.pos_bound[:2].max()
    assert (o["pos"][2:] == POISON).all() and (o["assoc"][2:] == IPOISON).all() and (o["cand_cell"][nc:] == IPOISON).all()


def test_nothing_above_min_score_writes_nothing(pkg, ctx):
    hand = np.full((5, 7), 1.0)
    hand[2, 3] = 2.0
    sc = _hand_scene(7, 5)
    st, o, ref = _run_on_map(pkg, ctx, sc, hand, fill=(POISON, IPOISON), minScore=2.5)
    assert st == 0 and o["n_out"].tolist() == [0, 0] and len(ref.cand_cell) == 0
    for k, v in o.items():
        if k != "n_out":
            assert (v == (POISON if v.dtype == np.float64 else IPOISON)).all(), k


# ---------------------------------------------------------------- 3
@pytest.mark.parametrize("name", list(R.CHAIN_SCENES))
def test_full_chain_against_the_restatement(pkg, ctx, name):
    sc = R.chain_scene(name)
    ref = sc.ref
    got = pkg.sensing.estimation.localizeTargets(sc.nodes, sc.links, sc.given, sc.grid, height=sc.height, return_map=True, return_candidates=True, ctx=ctx,
                                                 **{k: v for k, v in sc.par.items()})
    n = len(ref.pos)
    assert got["cand_cell"].tolist() == ref.cand_cell.tolist() and got["cand_status"].tolist() == ref.cand_status.tolist()
    assert got["assoc"].tolist() == ref.assoc.tolist() and got["n_links"].tolist() == ref.n_links.tolist() and got["vel_status"].tolist() == ref.vel_status.tolist()
    assert got["pos"].shape == (n, 2) and got["vel"].shape == (n, 2) and got["map"].shape == sc.ref_map.shape
    e_map = float(np.abs(got["map"].astype(R.LD) - sc.ref_map).max())
    e_cs = float(np.abs(got["cand_score"].astype(R.LD) - ref.cand_score).max()) if len(ref.cand_cell) else 0.0
    print(f"{name}: statuses {got['cand_status'].tolist()[:10]}.., {n} targets; map error {e_map:.3e}, candidate score error {e_cs:.3e} (bound {sc.bound:.3e})")
    assert e_map <= sc.bound and e_cs <= sc.bound
    if n:
        e_pos = np.abs(got["pos"].astype(R.LD) - ref.pos).max(axis=1).astype(np.float64)
        e_rms = np.abs(got["rms"].astype(R.LD) - ref.rms).astype(np.float64)
        e_s = np.abs(got["score"].astype(R.LD) - ref.score).astype(np.float64)
        ok = ref.vel_status == 0
        e_vel = np.abs(got["vel"][ok].astype(R.LD) - ref.vel[ok]).max(axis=1).astype(np.float64) if ok.any() else np.zeros(0)
        print(f"{name}: position errors {e_pos.tolist()} m (bounds {ref.pos_bound.tolist()}), velocity errors {e_vel.tolist()} (bounds {ref.vel_bound[ok].tolist()}), "
              f"rms errors {e_rms.tolist()} (bounds {ref.rms_bound.tolist()}); positions {got['pos'].tolist()}, velocities {got['vel'].tolist()}")
        assert (e_pos <= ref.pos_bound).all() and (e_rms <= ref.rms_bound).all() and (e_s <= sc.bound).all() and (e_vel <= ref.vel_bound[ok]).all()
        assert np.isnan(got["vel"][~ok]).all()
    want = {"status_1": 1, "status_2": 2, "status_3": 3}.get(name)
    if want:
        assert want in got["cand_status"].tolist()
    if name == "one_doppler":
        assert n == 4 and np.isnan(got["vel"]).all() and (got["vel_status"] == 1).all()


# ---------------------------------------------------------------- 4
def _base():
    """Three nodes, two links, three measurements given sorted, a 5 x 3 grid."""
    nodes = np.array([[0.0, 0.0, 25.0], [80.0, 0.0, 25.0], [40.0, 64.0, 30.0]])
    links = [(0, 1), (2, 2)]
    meas = dict(link=np.array([0, 0, 1], dtype=np.int32), r=np.array([100.0, 102.0, 106.0]), s=np.array([1.0, np.nan, 2.0]), azi=np.array([10.0, np.nan, -103.0]),
                sigma_r=np.full(3, 2.0), sigma_v=np.ones(3), sigma_a=np.full(3, 2.0))
    return nodes, links, meas, (30.0, 4.0, 5, 20.0, 4.0, 3), 1.5


# name -> ({argument index: value}, {(argument index, element): value}); argument indices as in include/isac_localize.h, 0 = ctx
A_NODES, A_N, A_LTX, A_LRX, A_K, A_LINK, A_R, A_S, A_AZI, A_SR, A_SV, A_SA, A_M, A_X0, A_DX, A_NX, A_Y0, A_DY, A_NY, A_Z, A_MAP = range(1, 22)
A_MAXCAND, A_MINLINKS, A_GATE, A_ITERS, A_MAXMOVE, A_MAXT = 23, 24, 25, 26, 27, 28
SCENE_REFUSALS = {
    "n_nodes_65": ({A_N: 65}, {}), "n_nodes_0": ({A_N: 0}, {}), "n_links_257": ({A_K: 257}, {}), "n_links_0": ({A_K: 0}, {}), "n_meas_4097": ({A_M: 4097}, {}),
    "n_meas_0": ({A_M: 0}, {}), "nx_8193": ({A_NX: 8193}, {}), "ny_8193": ({A_NY: 8193}, {}), "nx_0": ({A_NX: 0}, {}), "ny_negative": ({A_NY: -1}, {}),
    "node_nan": ({}, {(A_NODES, 4): np.nan}), "node_inf": ({}, {(A_NODES, 8): np.inf}), "r_nan": ({}, {(A_R, 1): np.nan}), "r_inf": ({}, {(A_R, 0): -np.inf}),
    "sigma_r_zero": ({}, {(A_SR, 2): 0.0}), "sigma_r_negative": ({}, {(A_SR, 0): -1.0}), "sigma_v_nan": ({}, {(A_SV, 1): np.nan}), "sigma_v_zero": ({}, {(A_SV, 1): 0.0}),
    "sigma_a_inf": ({}, {(A_SA, 0): np.inf}), "sigma_a_zero": ({}, {(A_SA, 1): 0.0}), "azi_inf": ({}, {(A_AZI, 0): np.inf}),
    "dx_zero": ({A_DX: 0.0}, {}), "dy_negative": ({A_DY: -4.0}, {}), "dx_nan": ({A_DX: np.nan}, {}), "dy_inf": ({A_DY: np.inf}, {}), "x0_inf": ({A_X0: np.inf}, {}),
    "y0_nan": ({A_Y0: np.nan}, {}), "z_nan": ({A_Z: np.nan}, {}),
    "link_tx_out_of_range": ({}, {(A_LTX, 1): 3}), "link_rx_negative": ({}, {(A_LRX, 0): -1}), "meas_link_out_of_range": ({}, {(A_LINK, 2): 2}),
    "meas_link_negative": ({}, {(A_LINK, 0): -1}), "meas_link_not_sorted": ({}, {(A_LINK, 1): 1, (A_LINK, 2): 0}),
    **{f"null_{i}": ({i: None}, {}) for i in (A_NODES, A_LTX, A_LRX, A_LINK, A_R, A_S, A_AZI, A_SR, A_SV, A_SA, A_MAP)},
}
LOCALIZE_REFUSALS = {"max_cand_257": ({A_MAXCAND: 257}, {}), "max_cand_0": ({A_MAXCAND: 0}, {}), "max_targets_257": ({A_MAXT: 257}, {}), "max_targets_0": ({A_MAXT: 0}, {}),
                     "iters_65": ({A_ITERS: 65}, {}), "iters_negative": ({A_ITERS: -1}, {}), "gate_nan": ({A_GATE: np.nan}, {}), "max_move_inf": ({A_MAXMOVE: np.inf}, {}),
                     "min_score_nan": ({22: np.nan}, {}), "min_links_negative": ({A_MINLINKS: -1}, {}), **{f"null_out_{i}": ({i: None}, {}) for i in (29, 30, 31, 32, 33, 34, 35, 39)}}


def _raw_calls(pkg, ctx, brk):
    """Both calls on the base scene with one thing broken, a poisoned device map and poisoned host outputs: (status of the map call, its map afterwards, status of the
    localize call, its outputs)."""
    args_brk, elem_brk = brk
    scene = _mod(pkg).Scene(*_base())
    arrs = {A_NODES: scene.nodes.reshape(-1), A_LTX: scene.link_tx, A_LRX: scene.link_rx, A_LINK: scene.link, **{A_R + i: a for i, a in enumerate(scene.f)}}
    for (i, e), v in elem_brk.items():
        arrs[i][e] = v
    d_map = ctx.to_device(np.full((5, 3), POISON, order="F"))
    try:
        a = list(scene.args(ctx, d_map))
        T, Cn = 4, 4
        o = dict(pos=np.full((T, 2), POISON), vel=np.full((T, 2), POISON), vel_status=np.full(T, IPOISON, dtype=np.int32), score=np.full(T, POISON),
                 n_links=np.full(T, IPOISON, dtype=np.int32), assoc=np.full((T, 2), IPOISON, dtype=np.int32), rms=np.full(T, POISON), cand_cell=np.full(Cn, IPOISON, dtype=np.int32),
                 cand_score=np.full(Cn, POISON), cand_status=np.full(Cn, IPOISON, dtype=np.int32), n_out=np.full(2, IPOISON, dtype=np.int32))
        b = a + [0.5, Cn, 1, 4.0, 4, 16.0, T] + [v.ctypes.data_as(C.c_void_p) for v in o.values()]
        for i, v in args_brk.items():
            b[i] = v
            if i < len(a):
                a[i] = v
        st_map = ctx.lib.isac_position_map_dev(*a)
        ctx.sync()
        after = d_map.numpy()
        if st_map == 0:                                                     # the valid call: give the localize call a clean poisoned map too
            ctx.check(ctx.lib.isac_memcpy_h2d(ctx.handle, d_map, np.full((5, 3), 1.0, order="F").ctypes.data_as(C.c_void_p), d_map.nbytes))
        st_loc = ctx.lib.isac_localize_dev(*b)
        ctx.sync()
    finally:
        d_map.free()
    return st_map, after, st_loc, o


def _untouched(o):
    return all((v == (POISON if v.dtype == np.float64 else IPOISON)).all() for v in o.values())


@pytest.mark.parametrize("name", list(SCENE_REFUSALS))
def test_refused_scenes_write_nothing(pkg, ctx, name):
    st_map, after, st_loc, o = _raw_calls(pkg, ctx, SCENE_REFUSALS[name])
    msg = (ctx.lib.isac_last_error(ctx.handle) or b"").decode()
    print(f"{name}: {st_map}, {st_loc} ({msg})")
    assert st_map == 1 and st_loc == 1, msg
    assert (after == POISON).all() and _untouched(o)


@pytest.mark.parametrize("name", list(LOCALIZE_REFUSALS))
def test_refused_localize_calls_write_nothing(pkg, ctx, name):
    st_map, after, st_loc, o = _raw_calls(pkg, ctx, LOCALIZE_REFUSALS[name])
    msg = (ctx.lib.isac_last_error(ctx.handle) or b"").decode()
    print(f"{name}: {st_loc} ({msg})")
    assert st_map == 0 and st_loc == 1, msg
    assert _untouched(o)


def test_the_refusal_shape_unbroken_is_accepted(pkg, ctx):
    st_map, after, st_loc, o = _raw_calls(pkg, ctx, ({}, {}))
    assert st_map == 0 and st_loc == 0 and np.isfinite(after).all() and (after >= 0).all() and (after <= 2.0).all()
    assert o["n_out"][1] == 1 and o["cand_cell"][0] == 0 and o["cand_score"][0] == 1.0 and o["cand_status"][0] in (0, 1, 2, 3)   # the map of ones: a plateau, its lowest index
    assert o["n_out"][0] == (o["cand_status"][0] == 0) and (o["cand_cell"][1:] == IPOISON).all()


# ---------------------------------------------------------------- 5
def test_the_context_keeps_its_cpi_and_a_pending_submit(pkg):
    """A completed CPI's list, detections, power window, covariance and spectrum, and then a submitted, uncollected CPI, on the context that localises in between."""
    import _subsample_restatement as S
    F = import_module(pkg.__name__ + ".sensing.estimation.fft2D")
    sc = S.e2e_scene()
    loc = R.chain_scene("three_nodes")
    c = pkg.Context()
    try:
        rp = pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)
        cf = pkg.sensing.detection.cfar2D(rp)
        targets = [SimpleNamespace(position=np.asarray(p, dtype=np.float64), velocity=np.zeros(3), rcs=1.0) for p in sc.cell.targetPosition]
        paths = pkg.sensing.channelModels.multiStaticPaths(sc.cell, [sc.cell], targets, subSample=True, carrierInfo=sc.carrier, waveInfo=sc.wave)
        d_wave, d_txg = c.to_device(sc.tx_wave), c.to_device(sc.tx_grid)
        echo = pkg.sensing.multiStaticSensing([d_wave], sc.tx_grid.shape, sc.carrier, rp, paths, seed=S.E2E_SEED, noise_domain="spectral", nfft=sc.wave.Nfft, ctx=c)
        pkg.sensing.estimation.fft2D(rp, cf, echo, d_txg, ctx=c)
        tl, dbg = pkg.sensing.estimation.targetList(c, snapshots=True), F.fft2D_debug(c, sc.A)
        run = lambda: pkg.sensing.estimation.localizeTargets(loc.nodes, loc.links, loc.given, loc.grid, height=loc.height, ctx=c)   # noqa: E731
        want = run()
        tl_after, dbg_after = pkg.sensing.estimation.targetList(c, snapshots=True), F.fft2D_debug(c, sc.A)
        assert sorted(tl) == sorted(tl_after) and tl["row"].size >= 1 and len(want["pos"]) == 4
        for k in tl:
            assert np.asarray(tl[k]).tobytes() == np.asarray(tl_after[k]).tobytes(), k
        for a, b in zip(dbg.detections + dbg.det_pow, dbg_after.detections + dbg_after.det_pow):
            assert a.tobytes() == b.tobytes()
        for k in ("power_window", "Ra", "spectrum_db"):
            assert getattr(dbg, k).tobytes() == getattr(dbg_after, k).tobytes(), k
        ref = pkg._lib.EstResult()
        F.fft2D_submit(rp, cf, echo, d_txg, ctx=c)
        c.check(c.lib.isac_fft2d_collect(c.handle, C.byref(ref)))
        F.fft2D_submit(rp, cf, echo, d_txg, ctx=c)
        got = run()
        res = pkg._lib.EstResult()
        c.check(c.lib.isac_fft2d_collect(c.handle, C.byref(res)))
        assert ref.n_rng >= 1 and bytes(res) == bytes(ref)
        for k in want:
            assert want[k].tobytes() == got[k].tobytes(), k
    finally:
        c.close()


# ---------------------------------------------------------------- 6
E2E_TARGETS = ((120.0, 160.0, 1.5), (140.0, 400.0, 1.5))                    # both on one side of the baseline between the cells; the grid leaves their mirror images out
E2E_VELOCITY = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))                          # at rest: every link sees both on a Doppler bin (the bins are 43 m/s wide at 28 symbols)
E2E_NEIGHBOUR = (400.0, 120.0, 30.0)
E2E_GRID = (0.0, 2.0, 201, 130.0, 2.0, 161)                                 # x 0 .. 400, y 130 .. 450: above the baseline y = 0.3 x where the targets are


def test_end_to_end_two_cells_two_targets(pkg):
    """Two cells, two targets, a wall on the direct path (directLoS = [1, 0]); each cell receives its own echo and the other's transmission off the targets, and forms
    one list with its own transmit grid and one with the neighbour's: four links.  Range sums only (a ULA cannot tell front from back, and the neighbour sees the targets
    behind its broadside); the grid covers one side of the baseline."""
    from conftest import make_scene
    est = pkg.sensing.estimation
    cells = []
    for i, pos in enumerate((None, E2E_NEIGHBOUR)):
        sc = make_scene(n_ants=4, n_slots=2, nrb=24, targets=E2E_TARGETS, velocity=(0.0, 0.0), seed=31 + i, zero_s_slots=False, with_noise=False, num_slots_param=6)
        if pos is not None:
            sc.cell.gNBPosition = np.array(pos)
        cells.append(sc)
    targets = [SimpleNamespace(position=np.array(p), velocity=np.array(v), rcs=1.0) for p, v in zip(E2E_TARGETS, E2E_VELOCITY)]
    nodes = np.array([np.asarray(sc.cell.gNBPosition, dtype=np.float64) for sc in cells])
    links = [(0, 0), (1, 0), (0, 1), (1, 1)]                                # (tx node, rx node)
    c = pkg.Context()
    try:
        d_wave, d_txg = [c.to_device(sc.tx_wave) for sc in cells], [c.to_device(sc.tx_grid) for sc in cells]
        lists = {}
        for rx in (0, 1):
            sc, other = cells[rx], 1 - rx
            rp = pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)
            cf = pkg.sensing.detection.cfar2D(rp)
            paths = pkg.sensing.channelModels.multiStaticPaths(sc.cell, [sc.cell, cells[other].cell], targets, carrierInfo=sc.carrier, waveInfo=sc.wave, directLoS=[1, 0],
                                                               subSample=True)
            echo = pkg.sensing.multiStaticSensing([d_wave[rx], d_wave[other]], sc.tx_grid.shape, sc.carrier, rp, paths, seed=4242 + rx, noise_domain="spectral",
                                                  nfft=sc.wave.Nfft, ctx=c)
            for tx in (rx, other):
                est.fft2D(rp, cf, echo, d_txg[tx], ctx=c)
                fine = est.refineTargets(c, est.targetList(c, snapshots=True), snapshots=True)
                lists[(tx, rx)] = est.refineRange(c, echo, d_txg[tx], rp, fine)
                print(f"link tx {tx} -> rx {rx}: rng {lists[(tx, rx)]['rng'].tolist()}, vel {lists[(tx, rx)]['vel'].tolist()}, sidelobe_of {fine['sidelobe_of'].tolist()}")
        r_res = float(rp.rRes)
        meas = est.linkMeasurements([lists[k] for k in links], links, rp, useAzimuth=False)
        got = est.localizeTargets(nodes, links, meas, E2E_GRID, height=1.5, return_candidates=True, ctx=c)
    finally:
        c.close()
    sc = R.make_scene(nodes, links, meas, E2E_GRID, 1.5)
    ref = R.localize(sc, R.position_map(sc), **R.DEFAULTS)
    bound = R.map_bound(sc)[0]
    rmse = pkg.sensing.postProcessing.getPositionRMSE(got, np.array(E2E_TARGETS), r_res)
    true_r = [[float(np.linalg.norm(np.array(p) - nodes[t]) + np.linalg.norm(np.array(p) - nodes[r])) for p in E2E_TARGETS] for t, r in links]
    print(f"end to end: range sums {meas['r'].tolist()} on links {meas['link'].tolist()} (truth per link {true_r}); positions {got['pos'].tolist()} for {E2E_TARGETS}: "
          f"errors {rmse.posRMSE.tolist()} m (rRes {r_res:.3f} m), matches {rmse.match.tolist()}; n_links {got['n_links'].tolist()}, rms {got['rms'].tolist()}, candidate statuses "
          f"{got['cand_status'].tolist()}; margins {ref.margins}, map bound {bound:.3e}")
    assert bound <= 1e-10 and all(ref.margins[k] > 1e4 * bound for k in ref.margins)
    assert got["cand_cell"].tolist() == ref.cand_cell.tolist() and got["cand_status"].tolist() == ref.cand_status.tolist() and got["assoc"].tolist() == ref.assoc.tolist()
    assert (np.abs(got["pos"].astype(R.LD) - ref.pos).max(axis=1) <= ref.pos_bound).all() and (ref.pos_bound <= 1e-8).all()
    assert len(got["pos"]) == 2
    assert sorted(rmse.match.tolist()) == [0, 1] and (rmse.posRMSE < r_res).all()
