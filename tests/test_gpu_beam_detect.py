"""isac_fft2d_get_rdm_window / isac_fft2d_beam_detect on the MI355X: the complex window of the last fft2D and CFAR on beam planes of it (project-defined --
include/isac_beams.h).

Scenes, beam sets, cases and the oracle-only results come from tests/_beam_detect_restatement.py; tests/test_beam_detect_cpu.py has shown on the oracle that every
decision of every case clears the 1e-9 guard band, so nothing here is left out or skipped.  273-PRB scenes have L = 56 symbols, 24-PRB scenes L = 28.
One refusal is not provoked here: nr nc n_beams >= 2^31.  With n_beams <= ISAC_MAX_BEAMS = 1024 (more is refused first) it needs a window of at least 2^21 cells, and
the fft2D that would have to leave such a window is itself refused by the CFAR stage (a CUT zone of that many rows does not fit its LDS-staged detector)."""
from __future__ import annotations

import ctypes as C
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import make_scene

import _beam_detect_restatement as R
import _cfar_methods_restatement as M

pytestmark = pytest.mark.gpu

LIST_KEYS = ("row", "col", "hits", "power", "rng", "vel", "azi", "beam")
CASE_IDS = ["-".join(map(str, c)) for c in R.CASES]
SCENE_NAMES = list(dict.fromkeys(c[0] for c in R.CASES))
INVALID_ARG, UNSUPPORTED = 1, 7


def _same_list(a, b):
    assert a["n_total"] == b["n_total"]
    for k in LIST_KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k


def _blocks(pkg, sc):
    rp = pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)
    return rp, pkg.sensing.detection.cfar2D(rp)


def _fft2d(pkg, ctx, rp, cf, echo, d_txg, **kw):
    """fft2D; a planar array with ISAC_OPT_UPA_DOA off answers UNSUPPORTED for its own DoA stage after it has collected the CPI (the calls under test do not depend on the option)."""
    try:
        return pkg.sensing.estimation.fft2D(rp, cf, echo, d_txg, ctx=ctx, **kw)
    except pkg.IsacError as e:
        if not (e.name == "UNSUPPORTED" and getattr(rp.antennaType, "kind", "ula") == "upa"):
            raise
        return None


_scenes, _cases = {}, {}


@pytest.fixture(scope="module")
def runs(pkg):
    """scene name -> its run, made on first use: a context of its own (the completed CPI stays on it for every case of the scene), the getters before the calls under test,
    the complex window, the per-target list with snapshots."""
    F = import_module(pkg.__name__ + ".sensing.estimation.fft2D")

    def get(name):
        if name not in _scenes:
            sc = R.make(name)
            rp, cf = _blocks(pkg, sc)
            cf.cfarDetector2D.GuardBandSize, cf.cfarDetector2D.TrainingBandSize = R.bands_of(name)     # the default bands for every scene but the asymmetric one
            ctx = pkg.Context()
            d_txg, d_wave = ctx.to_device(sc.tx_grid), ctx.to_device(sc.tx_wave)
            echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=ctx)
            est = _fft2d(pkg, ctx, rp, cf, echo, d_txg)
            upa = getattr(rp.antennaType, "kind", "ula") == "upa"
            dbg = F.fft2D_debug(ctx, sc.A)
            tl = (pkg.sensing.estimation.targetListUPA if upa else pkg.sensing.estimation.targetList)(ctx, snapshots=True)
            Y, fr, fc = pkg.sensing.estimation.rdmWindow(ctx)
            _scenes[name] = SimpleNamespace(sc=sc, rp=rp, cf=cf, ctx=ctx, est=est, dbg=dbg, tl=tl, Y=Y, first_row=fr, first_col=fc, rect=F._cut_rectangle(cf.CUTIdx),
                                            keep=(echo, d_txg, d_wave))
        return _scenes[name]

    yield get
    for r in _scenes.values():
        r.ctx.close()
    _scenes.clear()
    _cases.clear()


def _case(pkg, runs, case):
    """beamDetect of a case with its debug output, once per module."""
    if case not in _cases:
        name, beams, method, rank = case
        r = runs(name)
        W, azi = R.weights(r.sc, beams)
        res, dbg = pkg.sensing.estimation.beamDetect(r.ctx, W, Method=method, Rank=rank, beamAzimuth=azi, return_debug=True)
        _cases[case] = SimpleNamespace(r=r, W=W, azi=azi, res=res, dbg=dbg)
    return _cases[case]


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_rdm_window(pkg, runs, name):
    """Y against the oracle's complex window to 1e-10 of max |rdm| (the project's field tolerance); the per-target list's snapshots are Y at the listed cells, byte for
    byte (one device definition of the per-cell chain)."""
    r, w = runs(name), R.oracle_window(name)
    assert r.Y.shape == w.win.shape and (r.first_row, r.first_col) == (w.first_row, w.first_col) == (r.dbg.first_row, r.dbg.first_col)
    err = np.abs(r.Y - w.win).max() / w.rdm_max
    print(f"{name}: window {r.Y.shape}, error {err:.3e} of max |rdm|; {r.tl['n_total']} listed cells")
    assert err <= 1e-10
    assert r.tl["n_total"] >= 1
    at = r.Y[r.tl["row"] - r.first_row, r.tl["col"] - r.first_col, :].T
    assert np.asfortranarray(at).tobytes(order="F") == r.tl["snapshots"].tobytes(order="F")


@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
def test_beam_planes(pkg, runs, case):
    """beam_pow against the restatement's step 2 on the device's own Y: 1e-10 of each plane's maximum."""
    c = _case(pkg, runs, case)
    want = R.beam_planes(c.r.Y, c.W)
    got = c.dbg.beam_pow
    assert got.shape == want.shape
    err = (np.abs(got - want).max(axis=(0, 1)) / want.max(axis=(0, 1))).max()
    print(f"{case}: {got.shape[2]} planes, error {err:.3e} of the plane maximum")
    assert err <= 1e-10


@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
def test_lists_equal_the_restatement_on_the_devices_own_planes(pkg, runs, case):
    """Kernel level, exact: steps 3 and 4 of the restatement on the device's own beam planes give the device's per-beam lists, hits, row, col, beam and power (bytes)."""
    c = _case(pkg, runs, case)
    r, (_, _, method, rank) = c.r, case
    guard, train = R.bands_of(case[0])
    alpha = M.threshold_factor(method, M.n_train(guard, train), float(r.rp.Pfa), rank)
    want = R.beam_detect_on_planes(c.dbg.beam_pow, r.first_row, r.first_col, r.rect, guard, train, method, alpha, rank, r.rp)
    res = c.res
    print(f"{case}: {res['n_total']} targets, {c.dbg.totalDetections} detections; rows {res['row'][:6].tolist()} cols {res['col'][:6].tolist()} beam {res['beam'][:6].tolist()}")
    assert len(c.dbg.detections) == len(want.detections) == c.W.shape[1]
    for got_d, got_p, want_d, want_p in zip(c.dbg.detections, c.dbg.det_pow, want.detections, want.det_pow):
        assert np.array_equal(got_d, want_d) and got_p.tobytes() == want_p.tobytes()
    assert res["n_total"] == want.row.size >= 1
    for k in ("row", "col", "hits", "beam"):
        assert np.array_equal(res[k], getattr(want, k)), k
    assert res["power"].tobytes() == want.power.tobytes()
    assert np.array_equal(res["rng"], want.rng) and np.array_equal(res["vel"], want.vel) and np.array_equal(res["azi"], c.azi[want.beam - 1])


@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
def test_chain_equals_the_oracle_only_result(pkg, runs, case):
    c, t = _case(pkg, runs, case), R.oracle_beam_detect(*case)
    res = c.res
    assert res["n_total"] == t.row.size
    for k in ("row", "col", "hits", "beam", "rng", "vel", "azi"):
        assert np.array_equal(res[k], getattr(t, k)), k
    assert len(c.dbg.detections) == len(t.detections)
    for got_d, want_d in zip(c.dbg.detections, t.detections):
        assert np.array_equal(got_d, want_d)
    print(f"{case}: power error {np.abs(res['power'] / t.power - 1).max():.3e} relative")
    assert (np.abs(res["power"] - t.power) <= 1e-10 * t.power).all()


def test_weak_target_is_listed_by_the_matched_beam_only(pkg, runs):
    """a8_273prb with the second target's amplitude x 0.1: fft2D on the device reports no antenna hit at (152, 124) and no 184.2 m in rngEst; beamDetect with the weight
    matched to target 2 lists that cell, with beam 1."""
    r = runs(R.WEAK)
    cell = (152, 124)
    rng_cell = (cell[0] - 1) * r.rp.rRes
    assert abs(rng_cell - 184.2) < 0.05
    assert len(r.dbg.detections) == 8 and not any(((d[0] == cell[0]) & (d[1] == cell[1])).any() for d in r.dbg.detections)
    assert not np.any(np.abs(r.est.rngEst - rng_cell) < 0.5 * r.rp.rRes)
    azi, _ = R.target_direction(r.sc, 1)
    W = pkg.sensing.estimation.beamWeights(r.rp, azi)
    res = pkg.sensing.estimation.beamDetect(r.ctx, W)
    i = np.flatnonzero((res["row"] == cell[0]) & (res["col"] == cell[1]))
    print(f"rngEst {r.est.rngEst.tolist()}; beam list rows {res['row'].tolist()} cols {res['col'].tolist()} rng {res['rng'].tolist()} beam {res['beam'].tolist()}")
    assert i.size == 1 and res["beam"][i[0]] == 1 and res["hits"][i[0]] == 1 and res["azi"][i[0]] == 1.0 and res["rng"][i[0]] == rng_cell


def test_lazy_grid_gives_the_same_result(pkg):
    """8 x 8, A = 64, Q = 1, Philox spectral noise, L = 28 (~100 MB): the echo grid the context re-forms (never stored) against the stored one -- window, beam planes,
    per-beam lists and list byte for byte.  nFFT = 64 so that the 28-symbol scene has detections at all."""
    sc = make_scene(n_ants=64, n_slots=2, num_slots_param=6, with_noise=False, zero_s_slots=False, seed=31)
    sc.cell.gNBSenAntenna = SimpleNamespace(kind="upa", nV=8, nH=8, dV=0.5, dH=0.5)
    rp, cf = _blocks(pkg, sc)
    azi, ele = R.beam_set(sc, "b16")
    W = pkg.sensing.estimation.beamWeights(rp, azi, ele)
    est_mod = pkg.sensing.estimation
    c = pkg.Context()
    c.set_upa_doa(True)
    try:
        d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
        kw = dict(nfft=4096, fuse_fft2d=(rp, cf, d_txg), ctx=c, seed=77, noise_domain="spectral")
        arr = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, **kw)
        est_mod.fft2D(rp, cf, arr, d_txg, reuse_range=True, ctx=c)
        y0 = est_mod.rdmWindow(c)
        stored, dbg0 = est_mod.beamDetect(c, W, beamAzimuth=azi, return_debug=True)
        lz = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, lazy=True, **kw)
        est_mod.fft2D(rp, cf, lz, d_txg, reuse_range=True, ctx=c)
        y1 = est_mod.rdmWindow(c)
        lazy, dbg1 = est_mod.beamDetect(c, W, beamAzimuth=azi, return_debug=True)
        assert stored["n_total"] >= 1 and dbg0.totalDetections >= 1
        _same_list(lazy, stored)
        assert y0[1:] == y1[1:] and y0[0].tobytes(order="F") == y1[0].tobytes(order="F")
        assert dbg0.beam_pow.tobytes(order="F") == dbg1.beam_pow.tobytes(order="F")
        for a, b in zip(dbg0.detections + dbg0.det_pow, dbg1.detections + dbg1.det_pow):
            assert a.tobytes() == b.tobytes()
    finally:
        c.close()


def test_existing_getters_are_untouched_by_the_calls(pkg, runs):
    """Detections, power window, covariance, MUSIC spectrum and the per-target list byte-identical before and after rdmWindow / beamDetect; a pending submit and its result
    survive a (refused) call in between, and the collected CPI gives the beam list again."""
    case = ("a4_273prb", "b37", "CA", 1)
    c = _case(pkg, runs, case)
    r = c.r
    F = import_module(pkg.__name__ + ".sensing.estimation.fft2D")
    after = F.fft2D_debug(r.ctx, r.sc.A)
    for k in ("power_window", "Ra", "spectrum_db"):
        assert getattr(r.dbg, k).tobytes() == getattr(after, k).tobytes(), k
    assert (r.dbg.first_row, r.dbg.first_col) == (after.first_row, after.first_col)
    for a, b in zip(r.dbg.detections + r.dbg.det_pow, after.detections + after.det_pow):
        assert a.tobytes() == b.tobytes()
    tl = pkg.sensing.estimation.targetList(r.ctx, snapshots=True)
    for k in ("row", "col", "hits", "power", "rng", "vel", "azi", "snapshots"):
        assert tl[k].tobytes() == r.tl[k].tobytes(), k
    sc = r.sc
    ctx = pkg.Context()
    try:
        d_txg, d_wave = ctx.to_device(sc.tx_grid), ctx.to_device(sc.tx_wave)
        echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, r.rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=ctx)
        F.fft2D_submit(r.rp, r.cf, echo, d_txg, ctx=ctx)
        for call in (lambda: pkg.sensing.estimation.beamDetect(ctx, c.W), lambda: pkg.sensing.estimation.rdmWindow(ctx)):
            with pytest.raises(pkg.IsacError) as e:                         # submitted, not collected: no completed fft2D
                call()
            assert e.value.name == "INVALID_ARG"
        est = F.fft2D_collect(ctx)
        for k in ("rngEst", "velEst", "aziEst"):
            assert getattr(est, k).tobytes() == getattr(r.est, k).tobytes(), k
        _same_list(pkg.sensing.estimation.beamDetect(ctx, c.W, beamAzimuth=c.azi), c.res)
    finally:
        ctx.close()


def _raw(pkg, ctx, W, n_beams, method=0, rank=1, factor=0.0, w_null=False, m_null=False, out_null=False, beam_null=False):
    L = pkg._lib
    m, out = L.CfarMethod(method, rank, factor), L.TargetList()
    beam = np.zeros(L.ISAC_MAX_TARGETS, dtype=np.int32)
    n_total = C.c_int32(-1)
    w = np.asfortranarray(np.asarray(W, dtype=np.complex128))
    st = ctx.lib.isac_fft2d_beam_detect(ctx.handle, None if w_null else w.ctypes.data_as(C.c_void_p), n_beams, None, None if m_null else C.byref(m),
                                        None if out_null else C.byref(out), None if beam_null else beam.ctypes.data_as(C.c_void_p), None, None, 1 << 30, None,
                                        C.byref(n_total), None)
    return st, out, beam, n_total.value


def _completed_fft2d(pkg, c, sc, guard, train):
    """fft2D of `sc` on context c with the detector's bands replaced; a CPI without a detection is still a completed one (collect raises NO_DETECTION after it has
    recorded the CPI)."""
    rp, cf = _blocks(pkg, sc)
    cf.cfarDetector2D.GuardBandSize, cf.cfarDetector2D.TrainingBandSize = tuple(guard), tuple(train)
    d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
    echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c)
    try:
        pkg.sensing.estimation.fft2D(rp, cf, echo, d_txg, ctx=c)
    except pkg.IsacError as e:
        if e.name != "NO_DETECTION":
            raise
    return rp, (echo, d_txg, d_wave)


@pytest.mark.parametrize("guard,train", [((2, 0), (1, 0)), ((0, 2), (0, 1))])
def test_a_halo_of_zero_is_unsupported(pkg, guard, train):
    """guard + training = 0 in one dimension: fft2D completes (N = 2 training cells), the window carries no neighbours there, the local-maximum test cannot be made."""
    sc = R.make("a4_24prb_generic")
    W, _ = R.weights(sc, "b5")
    c = pkg.Context()
    try:
        _, keep = _completed_fft2d(pkg, c, sc, guard, train)
        dims = (C.c_int32 * 3)()
        c.check(c.lib.isac_fft2d_get_power_window(c.handle, None, 0, dims, None, None))
        rect = (6, 52, 30, 36)
        assert (dims[0], dims[1]) == (rect[1] - rect[0] + 1 + 2 * (guard[0] + train[0]), rect[3] - rect[2] + 1 + 2 * (guard[1] + train[1]))
        with pytest.raises(pkg.IsacError) as e:
            pkg.sensing.estimation.beamDetect(c, W)
        assert e.value.name == "UNSUPPORTED" and "isac_fft2d_beam_detect" in str(e.value) and "halo" in str(e.value)
        Y, _, _ = pkg.sensing.estimation.rdmWindow(c)                         # the window itself needs no halo
        assert Y.shape == tuple(dims) and np.isfinite(Y).all()
    finally:
        c.close()


def test_detector_limits_of_redetect_are_unsupported(pkg):
    """N = 33 x 33 - 1 = 1088 training cells (guard [0 0], training [16 16]; the CUT zone starts at 170 m so that the window stays inside the map): above
    ISAC_CFAR_MAX_TRAIN = 1024.  fft2D (CA) completes; beamDetect with GOCA, SOCA or OS answers UNSUPPORTED, the limit of isac_fft2d_redetect's detector; CA has no such
    limit and gives, on this band geometry too, exactly what the restatement gives on the device's own planes."""
    guard, train = (0, 0), (16, 16)
    assert M.n_train(guard, train) == 1088 > pkg._lib.ISAC_CFAR_MAX_TRAIN
    sc = make_scene(n_ants=4, n_slots=2, nrb=24, num_slots_param=6, seed=23, detection_area=[[170.0, 500.0], [-50.0, 50.0]], targets=((100.0, 20.0, 1.5), (178.0, -36.0, 1.5)),
                    velocity=(7.0, -9.0), zero_s_slots=False)
    W, azi = R.weights(sc, "b5")
    c = pkg.Context()
    try:
        rp, keep = _completed_fft2d(pkg, c, sc, guard, train)
        for method, rank in (("GOCA", 1), ("SOCA", 1), ("OS", 544)):
            with pytest.raises(pkg.IsacError) as e:
                pkg.sensing.estimation.beamDetect(c, W, Method=method, Rank=rank)
            assert e.value.name == "UNSUPPORTED" and "ISAC_CFAR_MAX_TRAIN" in str(e.value), method
            assert _raw(pkg, c, W, 5, method=pkg._lib.CFAR_METHODS[method], rank=rank)[0] == UNSUPPORTED
        res, dbg = pkg.sensing.estimation.beamDetect(c, W, beamAzimuth=azi, return_debug=True)
        Y, fr, fc = pkg.sensing.estimation.rdmWindow(c)
        rect = (18, 52, 30, 36)
        assert (fr, fc) == (rect[0] - 16, rect[2] - 16) and Y.shape == (35 + 32, 7 + 32, 4)
        alpha = M.threshold_factor("CA", 1088, float(rp.Pfa))
        want = R.beam_detect_on_planes(dbg.beam_pow, fr, fc, rect, guard, train, "CA", alpha, 1, rp)
        print(f"N = 1088, CA: {res['n_total']} targets, {dbg.totalDetections} detections; margin of the closest CUT {want.margin_det:.3e}")
        err = (np.abs(dbg.beam_pow - R.beam_planes(Y, W)).max(axis=(0, 1)) / dbg.beam_pow.max(axis=(0, 1))).max()
        assert err <= 1e-10
        for got_d, got_p, want_d, want_p in zip(dbg.detections, dbg.det_pow, want.detections, want.det_pow):
            assert np.array_equal(got_d, want_d) and got_p.tobytes() == want_p.tobytes()
        assert res["n_total"] == want.row.size
        for k in ("row", "col", "hits", "beam"):
            assert np.array_equal(res[k], getattr(want, k)), k
        assert res["power"].tobytes() == want.power.tobytes()
    finally:
        c.close()


def test_contract(pkg):
    """Every refusal that a completed fft2D at the default bands can meet, the capacity answer, and 'no completed fft2D' before any call, after a submit without collect
    and after the range stage has rewritten the range rows."""
    sc = R.make("a4_24prb_generic")
    rp, cf = _blocks(pkg, sc)
    W, azi = R.weights(sc, "b5")
    A = sc.A
    F = import_module(pkg.__name__ + ".sensing.estimation.fft2D")
    c = pkg.Context()
    try:
        assert _raw(pkg, c, W, 5)[0] == INVALID_ARG                           # before any fft2D
        assert c.lib.isac_fft2d_get_rdm_window(c.handle, None, 0, None, None, None) == INVALID_ARG
        d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
        echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c)
        F.fft2D_submit(rp, cf, echo, d_txg, ctx=c)
        assert _raw(pkg, c, W, 5)[0] == INVALID_ARG                           # submitted, not collected
        F.fft2D_collect(c)
        st, out, beam, n_total = _raw(pkg, c, W, 5)
        full = pkg.sensing.estimation.beamDetect(c, W)
        assert st == 0 and out.n_targets == out.n_total == full["n_total"] >= 2 and n_total >= 2
        assert np.array_equal(full["azi"], full["beam"].astype(np.float64))   # no labels: the beam number
        assert np.array_equal(beam[: out.n_targets], full["beam"]) and full["beam"].min() >= 1 and full["beam"].max() <= 5
        for kw in (dict(w_null=True), dict(m_null=True), dict(out_null=True), dict(beam_null=True)):
            assert _raw(pkg, c, W, 5, **kw)[0] == INVALID_ARG, kw
        assert _raw(pkg, c, W, 0)[0] == INVALID_ARG and _raw(pkg, c, W, -1)[0] == INVALID_ARG
        for bad in (0.0, np.nan, np.inf):                                     # a column with a zero / non-finite norm
            Wb = W.copy()
            Wb[:, 3] = bad
            assert _raw(pkg, c, Wb, 5)[0] == INVALID_ARG, bad
        assert _raw(pkg, c, W, 5, method=4)[0] == INVALID_ARG                 # the method block: the cases of isac_cfar2d
        assert _raw(pkg, c, W, 5, method=3, rank=0)[0] == INVALID_ARG and _raw(pkg, c, W, 5, method=3, rank=25)[0] == INVALID_ARG
        assert _raw(pkg, c, W, 5, factor=-1.0)[0] == INVALID_ARG and _raw(pkg, c, W, 5, factor=np.nan)[0] == INVALID_ARG
        big = np.ones((A, pkg._lib.ISAC_MAX_BEAMS + 1), dtype=np.complex128, order="F")
        assert _raw(pkg, c, big, pkg._lib.ISAC_MAX_BEAMS + 1)[0] == UNSUPPORTED
        # ISAC_ERR_CAPACITY with n_total set; the size query of the window and its capacity answer
        L = pkg._lib
        m, out2 = L.CfarMethod(0, 1, 0.0), L.TargetList()
        idx, nt = np.zeros((2, 1), dtype=np.int32, order="F"), C.c_int32(-1)
        assert c.lib.isac_fft2d_beam_detect(c.handle, W.ctypes.data_as(C.c_void_p), 5, None, C.byref(m), C.byref(out2), beam.ctypes.data_as(C.c_void_p),
                                            idx.ctypes.data_as(C.c_void_p), None, 1, None, C.byref(nt), None) == 6
        assert nt.value == n_total
        dims = (C.c_int32 * 3)()
        assert c.lib.isac_fft2d_get_rdm_window(c.handle, None, 0, dims, None, None) == 0 and dims[2] == A
        y = np.zeros(tuple(dims), dtype=np.complex128, order="F")
        assert c.lib.isac_fft2d_get_rdm_window(c.handle, y.ctypes.data_as(C.c_void_p), y.size - 1, dims, None, None) == 6
        with pytest.raises(ValueError):
            pkg.sensing.estimation.beamDetect(c, W[:-1])                      # A - 1 rows
        _same_list(pkg.sensing.estimation.beamDetect(c, W), full)             # and none of the refusals disturbed the CPI
        # the range stage alone on OTHER grids rewrites the range rows: no stale answer
        ep, cfb = import_module(pkg.__name__ + ".sensing._marshal").est_block(rp), F._cfar_block(cf)
        other = c.to_device(np.asfortranarray(sc.tx_grid[:, ::-1, :]))
        c.check(c.lib.isac_fft2d_range_stage_dev(c.handle, C.byref(ep), C.byref(cfb), other, d_txg, sc.K, sc.L, sc.A))
        assert _raw(pkg, c, W, 5)[0] == INVALID_ARG
        assert c.lib.isac_fft2d_get_rdm_window(c.handle, None, 0, None, None, None) == INVALID_ARG
    finally:
        c.close()
