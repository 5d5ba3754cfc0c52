"""Target tracking across CPIs on the MI355X (project-defined -- include/isac_track.h): isac_track_reset_dev, isac_track_step_dev and
isac_track_get_dev (csrc/track.hip) against the long-double restatement of tests/_track_restatement.py.  tests/test_track_cpu.py has shown without a GPU that on every scene
float64 and long double make the same integer decisions, agree to 1e-10 in x and in P (relative to its largest entry), and that no decision is closer than 1e4
discrepancies; the device tolerances below leave two orders of margin over that.
  1. every scene, every scan, every output: integers exact, x to 1e-8, P and nis to 1e-8 of the largest reference entry; two runs from the same reset give the same
     bits; isac_track_get_dev returns the last step's table byte for byte
  2. refusals leave a poisoned state block and poisoned host outputs untouched; the same call unbroken succeeds
  3. the context's last CPI, its getters' answers and a pending submit are the same bytes before and after a step
  4. end to end: two cells, four links, two slowly moving targets, seven scans through multiStaticSensing -> fft2D -> targetList -> refineTargets -> refineRange ->
     linkMeasurements -> localizeTargets -> trackMeasurements -> Tracker"""
from __future__ import annotations

import ctypes as C
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest

import _track_restatement as R
from test_track_cpu import TRACK_REFUSALS, _valid_call

pytestmark = pytest.mark.gpu

X_TOL = 1e-8
REL_TOL = 1e-8
TABLE_INTS = ("status", "id", "age", "hits", "misses", "dof")


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context()
    yield c
    c.close()


def _tracker(pkg, ctx, sc):
    p = sc.par
    return pkg.sensing.estimation.Tracker(sc.nodes, sc.links, banks=sc.B, maxTracks=sc.T, height=sc.height, sigmaAcc=p["sigmaAcc"], gate=p["gate"], confirmHits=p["confirmHits"],
                                          tentMisses=p["tentMisses"], maxMisses=p["maxMisses"], initV0=p["initV0"], ctx=ctx)


def _run(pkg, ctx, sc):
    """The scene's scans on the device from a reset: the list of Tracker.step's outputs, and the table isac_track_get_dev returns at the end."""
    trk = _tracker(pkg, ctx, sc)
    try:
        outs = [trk.step(recs[0] if sc.B == 1 else recs, dt) for dt, recs in sc.scans]
        return outs, trk.table()
    finally:
        trk.close()


def _compare(got, ref, B):
    """One scan: the integers exact; returns (x error, P error / largest |P|, nis error / largest nis)."""
    for k in TABLE_INTS + ("n_confirmed",):
        assert np.array_equal(got[k], getattr(ref, k)), k
    assoc, kind = (got["assoc"], got["assoc_kind"]) if B > 1 else ([got["assoc"]], [got["assoc_kind"]])
    for b in range(B):
        assert np.array_equal(assoc[b], ref.assoc[b]) and np.array_equal(kind[b], ref.assoc_kind[b]), b
    assert np.array_equal(got["P"], np.swapaxes(got["P"], -1, -2))          # exactly symmetric
    ex = float(np.abs(got["x"].astype(R.LD) - ref.x).max())
    ep = float(np.abs(got["P"].astype(R.LD) - ref.P).max() / max(float(np.abs(ref.P).max()), 1e-300))
    en = float(np.abs(got["nis"].astype(R.LD) - ref.nis).max() / max(float(np.abs(ref.nis).max()), 1.0))
    return ex, ep, en


# ---------------------------------------------------------------- 1
@pytest.mark.parametrize("name", list(R.SCENES))
def test_scenes_against_the_restatement(pkg, ctx, name):
    sc, ref = R.scene(name), R.reference(name)
    outs, table = _run(pkg, ctx, sc)
    assert len(outs) == len(ref) >= 12
    worst = np.array([_compare(o, r, sc.B) for o, r in zip(outs, ref)]).max(axis=0)
    print(f"{name}: {len(outs)} scans, B {sc.B}, T {sc.T}: x error {worst[0]:.3e} (m, m/s), P error {worst[1]:.3e} and nis error {worst[2]:.3e} of the largest reference entry; "
          f"confirmed at the end {outs[-1]['n_confirmed'].tolist()[:8]}")
    assert worst[0] <= X_TOL and worst[1] <= REL_TOL and worst[2] <= REL_TOL
    for k in table:                                                         # the getter: the last step's table, byte for byte
        assert table[k].tobytes() == outs[-1][k].tobytes(), k
    again, _ = _run(pkg, ctx, sc)                                           # two runs from the same reset: the same bits
    for a, b in zip(outs, again):
        for k in a:
            for u, w in zip(a[k] if isinstance(a[k], list) else [a[k]], b[k] if isinstance(b[k], list) else [b[k]]):
                assert u.tobytes() == w.tobytes(), k


def test_track_targets_returns_the_history(pkg, ctx):
    """trackTargets on a scene: per scan the live tracks of the reference, in slot order; Tracker.tracks() the confirmed ones of the last scan."""
    sc, ref = R.scene("b1_t2_m3"), R.reference("b1_t2_m3")
    p = sc.par
    par = dict(banks=1, maxTracks=sc.T, height=sc.height, sigmaAcc=p["sigmaAcc"], gate=p["gate"], confirmHits=p["confirmHits"], tentMisses=p["tentMisses"],
               maxMisses=p["maxMisses"], initV0=p["initV0"])
    hist = pkg.sensing.estimation.trackTargets([recs[0] for _, recs in sc.scans], [dt for dt, _ in sc.scans], sc.nodes, sc.links, ctx=ctx, **par)
    assert len(hist) == len(ref)
    for h, r in zip(hist, ref):
        live = np.flatnonzero(r.status[0] > 0)
        t = h["tracks"][0]
        assert t["slot"].tolist() == live.tolist() and t["id"].tolist() == r.id[0][live].tolist() and t["status"].tolist() == r.status[0][live].tolist()
        assert np.abs(t["x"].astype(R.LD) - r.x[0][live]).max() <= X_TOL and h["n_confirmed"].tolist() == r.n_confirmed.tolist()
        assert np.array_equal(h["assoc"], r.assoc[0]) and np.array_equal(h["assoc_kind"], r.assoc_kind[0])
    trk = _tracker(pkg, ctx, sc)
    try:
        assert all(len(t["id"]) == 0 for t in trk.tracks(confirmedOnly=False))
        for dt, recs in sc.scans:
            trk.step(recs[0], dt)
        conf = np.flatnonzero(ref[-1].status[0] == 2)
        assert trk.tracks()[0]["id"].tolist() == ref[-1].id[0][conf].tolist() and trk.tracks(confirmedOnly=False)[0]["slot"].tolist() == np.flatnonzero(ref[-1].status[0] > 0).tolist()
        trk.reset()
        assert (trk.table()["status"] == 0).all() and trk.step(sc.scans[0][1][0], 0.0)["id"][0].max() == len(sc.scans[0][1][0]["group"]) - 1   # ids start again at 1: three fixes, two slots
    finally:
        trk.close()


# ---------------------------------------------------------------- 2
POISON = 0xA5


def _device_call(ctx, brk):
    """tests/test_track_cpu.py's call with the context, a poisoned device state block and poisoned host outputs, one thing broken: (status, state bytes afterwards, outputs)."""
    args, a, outs, _ = _valid_call()
    nbytes = int(ctx.lib.isac_track_state_bytes(2, 4))
    state = ctx.to_device(np.full(nbytes, POISON, dtype=np.uint8))
    try:
        args[0], args[1] = ctx.handle, state
        for (k, e), v in brk[1].items():
            a[k].reshape(-1)[e] = v
        for i, v in brk[0].items():
            args[i] = v
        for v in outs.values():
            v[...] = -7
        st = ctx.lib.isac_track_step_dev(*args)
        ctx.sync()
        return st, state.numpy(), outs
    finally:
        state.free()


@pytest.mark.parametrize("name", list(TRACK_REFUSALS))
def test_refused_calls_write_nothing(pkg, ctx, name):
    st, after, outs = _device_call(ctx, TRACK_REFUSALS[name])
    msg = (ctx.lib.isac_last_error(ctx.handle) or b"").decode()
    print(f"{name}: {st} ({msg})")
    assert st == 1, msg
    assert (after == POISON).all() and all((v == -7).all() for v in outs.values())


def test_the_refusal_shape_unbroken_is_accepted(pkg, ctx):
    args, a, outs, _ = _valid_call()
    nbytes = int(ctx.lib.isac_track_state_bytes(2, 4))
    state = ctx.to_device(np.full(nbytes, POISON, dtype=np.uint8))
    try:
        args[0], args[1] = ctx.handle, state
        ctx.check(ctx.lib.isac_track_reset_dev(ctx.handle, state, 2, 4))
        assert (state.numpy() == 0).all()
        ctx.check(ctx.lib.isac_track_step_dev(*args))
        assert outs["status"].tolist() == [1, 1, 0, 0, 0, 0, 0, 0] and outs["id"].tolist() == [1, 2, 0, 0, 0, 0, 0, 0] and outs["n_confirmed"].tolist() == [0, 0]
        assert outs["assoc"].tolist() == [0, 1, -1] and outs["assoc_kind"].tolist() == [2, 2, 0]
        assert outs["x"][:8].tolist() == [10.0, 20.0, 0.0, 1.0, 30.0, 40.0, 2.0, 0.0] and np.diag(outs["P"][:16].reshape(4, 4)).tolist() == [1.0, 1.0, 900.0, 1.0]
    finally:
        state.free()


# ---------------------------------------------------------------- 3
def test_the_context_keeps_its_cpi_and_a_pending_submit(pkg):
    """A completed CPI's list, detections, power window, covariance and spectrum, and then a submitted, uncollected CPI, on the context that tracks in between."""
    import _subsample_restatement as S
    F = import_module(pkg.__name__ + ".sensing.estimation.fft2D")
    sc = S.e2e_scene()
    tsc = R.scene("special")
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
        trk = _tracker(pkg, c, tsc)

        def run():
            trk.reset()
            return [trk.step(recs[0], dt) for dt, recs in tsc.scans[:4]][-1]
        want = run()
        tl_after, dbg_after = pkg.sensing.estimation.targetList(c, snapshots=True), F.fft2D_debug(c, sc.A)
        assert sorted(tl) == sorted(tl_after) and tl["row"].size >= 1 and want["n_confirmed"][0] == R.reference("special")[3].n_confirmed[0] >= 3
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
        trk.close()
    finally:
        c.close()


# ---------------------------------------------------------------- 4
E2E_TARGETS = ((120.0, 160.0, 1.5), (140.0, 400.0, 1.5))                    # tests/test_gpu_localize.py's two cells and two targets, here moving
E2E_VELOCITY = ((2.0, 1.0, 0.0), (-1.5, 2.0, 0.0))                          # a few m/s: every Doppler sum stays within a tenth of a bin of bin 0 (a bin is tens of m/s at 28 symbols), where DESIGN.md section 5 found every echo listed; targets between bins were not
E2E_NEIGHBOUR = (400.0, 120.0, 30.0)
E2E_GRID = (0.0, 2.0, 201, 130.0, 2.0, 161)
E2E_DT, E2E_SCANS = 1.0, 7


def test_end_to_end_two_cells_two_moving_targets(pkg):
    """Every scan places the targets at p + v t, synthesises both cells' echoes, forms the four links' lists, localises, and hands the fixes (group 0) and the link records
    (groups 1 .. 4) to the tracker.  The choice of velocities is verified on the lists: every link lists both echoes in every scan."""
    from conftest import make_scene
    est = pkg.sensing.estimation
    cells = []
    for i, pos in enumerate((None, E2E_NEIGHBOUR)):
        sc = make_scene(n_ants=4, n_slots=2, nrb=24, targets=E2E_TARGETS, velocity=(0.0, 0.0), seed=31 + i, zero_s_slots=False, with_noise=False, num_slots_param=6)
        if pos is not None:
            sc.cell.gNBPosition = np.array(pos)
        cells.append(sc)
    nodes = np.array([np.asarray(sc.cell.gNBPosition, dtype=np.float64) for sc in cells])
    links = [(0, 0), (1, 0), (0, 1), (1, 1)]
    par = dict(R.DEFAULTS)
    c = pkg.Context()
    records, truth, outs = [], [], []
    try:
        d_wave, d_txg = [c.to_device(sc.tx_wave) for sc in cells], [c.to_device(sc.tx_grid) for sc in cells]
        trk = est.Tracker(nodes, links, banks=1, maxTracks=8, height=1.5, ctx=c)
        for s in range(E2E_SCANS):
            t = E2E_DT * s
            pos = [np.array(p) + np.array(v) * t for p, v in zip(E2E_TARGETS, E2E_VELOCITY)]
            truth.append([[p[0], p[1], v[0], v[1]] for p, v in zip(pos, E2E_VELOCITY)])
            targets = [SimpleNamespace(position=p, velocity=np.array(v), rcs=1.0) for p, v in zip(pos, E2E_VELOCITY)]
            lists = {}
            for rx in (0, 1):
                sc, other = cells[rx], 1 - rx
                rp = pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)
                cf = pkg.sensing.detection.cfar2D(rp)
                paths = pkg.sensing.channelModels.multiStaticPaths(sc.cell, [sc.cell, cells[other].cell], targets, carrierInfo=sc.carrier, waveInfo=sc.wave, directLoS=[1, 0],
                                                                   subSample=True)
                echo = pkg.sensing.multiStaticSensing([d_wave[rx], d_wave[other]], sc.tx_grid.shape, sc.carrier, rp, paths, seed=4242 + rx + 2 * s, noise_domain="spectral",
                                                      nfft=sc.wave.Nfft, ctx=c)
                for tx in (rx, other):
                    est.fft2D(rp, cf, echo, d_txg[tx], ctx=c)
                    fine = est.refineTargets(c, est.targetList(c, snapshots=True), snapshots=True)
                    lists[(tx, rx)] = est.refineRange(c, echo, d_txg[tx], rp, fine)
            r_res, v_res = float(rp.rRes), float(rp.vRes)
            meas = est.linkMeasurements([lists[k] for k in links], links, rp, useAzimuth=False)
            true_r = [[float(np.linalg.norm(p - nodes[a]) + np.linalg.norm(p - nodes[b])) for p in pos] for a, b in links]
            print(f"scan {s}: range sums {meas['r'].round(2).tolist()} on links {meas['link'].tolist()} (truth per link {np.round(true_r, 2).tolist()}), Doppler sums {meas['s'].round(2).tolist()}")
            for k in range(4):                                              # the choice of velocities, verified: every link lists both echoes, each within rRes of its range sum
                rk = np.sort(meas["r"][meas["link"] == k])
                assert rk.size == 2 and np.abs(rk - np.sort(true_r[k])).max() < r_res, (s, k)
            fixes = est.localizeTargets(nodes, links, meas, E2E_GRID, height=1.5, ctx=c)
            rec = est.trackMeasurements(fixes, sigmaPos=r_res / 2.0, sigmaVel=v_res, links=meas)
            records.append(rec)
            outs.append(trk.step(rec, E2E_DT if s else 0.0))
            print(f"scan {s}: fixes {fixes['pos'].round(2).tolist()}; status {outs[-1]['status'][0].tolist()}, ids {outs[-1]['id'][0].tolist()}, x {outs[-1]['x'][0, :2].round(3).tolist()}")
        history = [dict(tracks=import_module(pkg.__name__ + ".sensing.estimation.trackTargets").tracks_of(o, confirmedOnly=False)) for o in outs]
        trk.close()
    finally:
        c.close()
    # ---- the device history equals the restatement on the same device lists
    st = R.new_state(1, 8)
    worst = np.zeros(3)
    for s, (rec, o) in enumerate(zip(records, outs)):
        ref = R.step(st, nodes, links, 1.5, par, [rec], E2E_DT if s else 0.0)
        worst = np.maximum(worst, _compare(o, ref, 1))
    truth = np.array(truth)
    rm = pkg.sensing.postProcessing.getTrackRMSE(history, truth, r_res)
    last = outs[-1]
    err = [float(np.hypot(*(last["x"][0, i, :2] - truth[-1, q, :2]))) for q in range(2) for i in np.flatnonzero((last["status"][0] == 2) & (last["id"][0] == rm.match[-1, q]))]
    print(f"end to end: device vs restatement x {worst[0]:.3e}, P {worst[1]:.3e}, nis {worst[2]:.3e}; matches per scan {rm.match.tolist()}; position RMSE {rm.posRMSE.tolist()} m, "
          f"velocity RMSE {rm.velRMSE.tolist()} m/s, id switches {rm.idSwitches}, false tracks {rm.falseTracks}; errors at the last scan {err} m (rRes {r_res:.3f} m, vRes {v_res:.3f} m/s)")
    assert worst[0] <= X_TOL and worst[1] <= REL_TOL and worst[2] <= REL_TOL
    for s, o in enumerate(outs):
        assert o["n_confirmed"][0] == (2 if s >= par["confirmHits"] - 1 else 0), s       # exactly one confirmed track per target from the third scan on, and no other
    assert (rm.match[par["confirmHits"] - 1:] > 0).all() and rm.idSwitches == 0 and rm.falseTracks == 0
    assert len(err) == 2 and max(err) < r_res
