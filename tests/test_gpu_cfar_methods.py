"""The GOCA / SOCA / OS detectors on the MI355X (include/isac_cfar.h: isac_cfar2d, isac_fft2d_redetect; project-defined).

Kernel level the comparisons are exact: the restatement (tests/_cfar_methods_restatement.py) runs on the very map the device detects on, with the threshold factor the
library's own host solver returns.  The chain against the oracle-only result runs the scene x method pairs tests/test_cfar_methods_cpu.py has cleared of the 1e-9 guard
band.  Scenes: tests/_target_list_restatement.py (the smallest at which fft2D detects anything)."""
from __future__ import annotations

import ctypes as C
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import load_pkg
from oracle.cfar import training_offsets

import _cfar_methods_restatement as M
import _target_list_restatement as R

pytestmark = pytest.mark.gpu

PANEL_ROWS = 32                          # kPanelRows of csrc/cfar.hip: CUT rows per workgroup
CODE = {"CA": 0, "GOCA": 1, "SOCA": 2, "OS": 3}
INVALID_ARG, CFAR_WINDOW, CAPACITY = 1, 5, 6


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context()
    yield c
    c.close()


def _alpha(pkg, method, n, pfa, rank):
    return pkg.sensing.detection.cfarThresholdFactor(method, n, pfa, Rank=rank)


# ---------------------------------------------------------------- isac_cfar2d
def _cfar2d(ctx, P, cuts, guard, train, pfa, method, rank=1, custom=0.0, cap=None, ca_entry=False):
    """(status, [2 x D] detections, n_det) of isac_cfar2d, or of isac_cfar2d_ca."""
    p = np.asfortranarray(P, dtype=np.float64)
    cut = np.asfortranarray(np.asarray(cuts, dtype=np.int32).reshape(2, -1))
    n_cut = cut.shape[1]
    cap = max(n_cut, 1) if cap is None else cap
    out = np.zeros((2, max(cap, 1)), dtype=np.int32, order="F")
    n_det = C.c_int32(-1)
    g, t = (C.c_int32 * 2)(*guard), (C.c_int32 * 2)(*train)
    head = (ctx.handle, p.ctypes.data_as(C.c_void_p), p.shape[0], p.shape[1], cut.ctypes.data_as(C.c_void_p), n_cut, g, t, pfa)
    tail = (out.ctypes.data_as(C.c_void_p), cap, C.byref(n_det))
    if ca_entry:
        st = ctx.lib.isac_cfar2d_ca(*head, *tail)
    else:
        st = ctx.lib.isac_cfar2d(*head, C.byref(_method_block(method, rank, custom)), *tail)
    return st, out[:, : max(min(n_det.value, cap), 0)].astype(np.int64), n_det.value


def _method_block(method, rank, custom):
    return load_pkg()._lib.CfarMethod(CODE[method] if isinstance(method, str) else method, rank, custom)


@pytest.fixture(scope="module")
def noise_map():
    rng = np.random.default_rng(11)
    P = rng.exponential(size=(40, 36))
    for (r, c), v in {(10, 9): 60.0, (13, 9): 25.0, (25, 20): 300.0, (25, 23): 40.0, (31, 30): 12.0, (6, 28): 9.0}.items():
        P[r - 1, c - 1] = v
    P[18 - 1, 14 - 1] = np.nan                                                 # in the training band of its neighbours, in the guard band of others
    return P


@pytest.mark.parametrize("guard,train", [((2, 2), (1, 1)), ((0, 0), (1, 1)), ((1, 0), (2, 1)), ((0, 1), (1, 0))])
def test_cfar2d_equals_the_restatement(pkg, ctx, noise_map, guard, train):
    """Every method (OS at ranks 1, N/2, N) and one custom factor; CUT lists of 1, 63, 65 and 300 entries in shuffled order, whose order the output keeps."""
    P, pfa = noise_map, 1e-2
    hr, hc = guard[0] + train[0], guard[1] + train[1]
    N = M.n_train(guard, train)
    allc = M.rectangle_cuts((hr + 1, 40 - hr, hc + 1, 36 - hc))
    rng = np.random.default_rng(5)
    n_seen = 0
    for n_cut in (1, 63, 65, 300):
        cuts = allc[:, rng.permutation(allc.shape[1])[:n_cut]]
        if n_cut == 1:
            cuts = np.array([[25], [20]])
        for method, rank, custom in [("CA", 1, 0.0), ("GOCA", 1, 0.0), ("SOCA", 1, 0.0), ("OS", 1, 0.0), ("OS", N // 2, 0.0), ("OS", N, 0.0), ("SOCA", 1, 3.25), ("OS", N // 2, 3.25)]:
            alpha = custom if custom else _alpha(pkg, method, N, pfa, rank)
            want = M.detect(P, cuts, guard, train, method, alpha, rank)
            st, got, n_det = _cfar2d(ctx, P, cuts, guard, train, pfa, method, rank, custom)
            assert st == 0 and n_det == want.shape[1], (n_cut, method, rank, custom)
            assert np.array_equal(got, want), (n_cut, method, rank, custom)
            n_seen += n_det
            if method == "CA":
                st2, ca, n_ca = _cfar2d(ctx, P, cuts, guard, train, pfa, method, ca_entry=True)
                assert st2 == 0 and n_ca == n_det and ca.tobytes() == got.tobytes()
    assert n_seen >= 16
    # no CUT that has the NaN among its training cells is detected by any method; some CUT next to it (NaN in its guard block) may be
    near = np.array([[18 + dr, 14 + dc] for dr, dc in training_offsets(guard, train)]).T
    near = near[:, (near[0] > hr) & (near[0] <= 40 - hr) & (near[1] > hc) & (near[1] <= 36 - hc)]
    for method in M.METHODS:
        st, got, n_det = _cfar2d(ctx, P, near, guard, train, 0.5, method, 1, 1e-6)        # a factor that would detect everything
        assert st == 0 and n_det == 0
    pkg_det = pkg.sensing.detection.cfarDetect(P, allc, SimpleNamespace(cfarDetector2D=pkg.sensing.detection.CFARDetector2D(pfa, guard, train)), Method="OS", Rank=N // 2, ctx=ctx)
    assert np.array_equal(pkg_det, M.detect(P, allc, guard, train, "OS", _alpha(pkg, "OS", N, pfa, N // 2), N // 2))


def test_cfar2d_errors(pkg, ctx, noise_map):
    P = noise_map
    g, t = (2, 2), (1, 1)
    for bad in ([[3], [10]], [[38], [10]], [[10], [3]], [[10], [34]]):          # the window leaves the map on each side
        assert _cfar2d(ctx, P, bad, g, t, 1e-2, "SOCA")[0] == CFAR_WINDOW
    allc = M.rectangle_cuts((4, 37, 4, 33))
    want = M.detect(P, allc, g, t, "OS", _alpha(pkg, "OS", 24, 1e-2, 18), 18)
    st, got, n_det = _cfar2d(ctx, P, allc, g, t, 1e-2, "OS", 18, cap=2)
    assert st == CAPACITY and n_det == want.shape[1] > 2 and np.array_equal(got, want[:, :2])
    for method, rank, custom, pfa in ((7, 1, 0.0, 1e-2), ("OS", 0, 0.0, 1e-2), ("OS", 25, 0.0, 1e-2), ("SOCA", 1, -1.0, 1e-2), ("SOCA", 1, float("nan"), 1e-2),
                                      ("GOCA", 1, 0.0, 0.0), ("GOCA", 1, 0.0, 1.0), ("OS", 25, 2.0, 1e-2)):
        assert _cfar2d(ctx, P, allc, g, t, pfa, method, rank, custom)[0] == INVALID_ARG, (method, rank, custom, pfa)
    assert _cfar2d(ctx, P, allc, g, t, 7.0, "SOCA", 1, 2.0)[0] == 0            # 'Custom': pfa is not used
    big = np.ones((64, 64))                                                    # N = 416 (guard [2 2], training [8 8]) works for every method
    big[31, 31] = 1e9                                                          # (OS rank 1 of 416 cells: alpha = 4.2e5)
    cuts = np.array([[32, 33], [32, 32]])
    for method, rank in (("CA", 1), ("GOCA", 1), ("SOCA", 1), ("OS", 1), ("OS", 312), ("OS", 416)):
        alpha = _alpha(pkg, method, 416, 1e-3, rank)
        st, got, n_det = _cfar2d(ctx, big, cuts, (2, 2), (8, 8), 1e-3, method, rank)
        assert st == 0 and np.array_equal(got, M.detect(big, cuts, (2, 2), (8, 8), method, alpha, rank)) and got.tolist() == [[32], [32]]


# ---------------------------------------------------------------- isac_fft2d_redetect
def _blocks(pkg, sc):
    rp = pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)
    return rp, pkg.sensing.detection.cfar2D(rp)


def _fft2d_mod(pkg):
    return import_module(pkg.__name__ + ".sensing.estimation.fft2D")


def _redetect_raw(pkg, ctx, A, method, rank=1, custom=0.0, cap=None):
    """isac_fft2d_redetect through ctypes: (status, namespace of everything it returns)."""
    L = pkg._lib
    m = L.CfarMethod(CODE[method] if isinstance(method, str) else method, rank, custom)
    res = L.EstResult()
    off = np.full(A + 1, -1, dtype=np.int32)
    n_total = C.c_int32(-1)
    st = ctx.lib.isac_fft2d_redetect(ctx.handle, C.byref(m), C.byref(res), None, None, 1 << 30, off.ctypes.data_as(C.c_void_p), C.byref(n_total))
    if st != 0:
        return st, None
    n = n_total.value
    cap = max(n, 1) if cap is None else cap
    idx = np.zeros((2, max(cap, 1)), dtype=np.int32, order="F")
    pw = np.zeros(max(cap, 1), dtype=np.float64)
    n_total = C.c_int32(-1)
    st = ctx.lib.isac_fft2d_redetect(ctx.handle, C.byref(m), C.byref(res), idx.ctypes.data_as(C.c_void_p), pw.ctypes.data_as(C.c_void_p), cap,
                                     off.ctypes.data_as(C.c_void_p), C.byref(n_total))
    return st, SimpleNamespace(res=res, idx=idx[:, :n], pw=pw[:n], off=off, n_total=n_total.value, rngEst=np.array(res.rng_est[: res.n_rng]),
                               velEst=np.array(res.vel_est[: res.n_vel]))


_runs = {}


def _run(pkg, ctx, name, rect=None):
    """Scene `name` (optionally with another CUT rectangle) through monoStaticSensing -> isac_fft2d_dev -> the getters, once per module (host copies only)."""
    key = (name, rect)
    if key not in _runs:
        sc = R.make(name)
        rp, cf = _blocks(pkg, sc)
        cf = R.with_bands(name, cf)                                            # the default bands for every scene but R.BAND_SCENE
        if rect is not None:
            cf = SimpleNamespace(CUTIdx=M.rectangle_cuts(rect), cfarDetector2D=cf.cfarDetector2D)
        d_txg, d_wave = ctx.to_device(sc.tx_grid), ctx.to_device(sc.tx_wave)
        echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=ctx)
        est, dbg = pkg.sensing.estimation.fft2D(rp, cf, echo, d_txg, return_debug=True, ctx=ctx)
        _runs[key] = SimpleNamespace(name=name, sc=sc, rp=rp, cf=cf, est=est, dbg=dbg, rect=_fft2d_mod(pkg)._cut_rectangle(cf.CUTIdx), grids=(echo, d_txg, d_wave))
    return _runs[key]


def _again(pkg, ctx, r):
    """The run's fft2D once more on `ctx` (another scene may have been there since)."""
    return pkg.sensing.estimation.fft2D(r.rp, r.cf, r.grids[0], r.grids[1], ctx=ctx)


def _check_against_restatement(pkg, ctx, r, method, rank, custom=0.0):
    g, t = R.bands_of(r.name)
    alpha = custom if custom else _alpha(pkg, method, M.n_train(g, t), float(r.rp.Pfa), rank)
    want = M.redetect(r.dbg.power_window, r.dbg.first_row, r.dbg.first_col, r.rect, g, t, method, alpha, rank, r.rp.rRes, r.rp.vRes, int(r.rp.nFFT))
    st, got = _redetect_raw(pkg, ctx, r.sc.A, method, rank, custom)
    assert st == 0
    assert got.n_total == want.totalDetections == got.res.total_detections and np.array_equal(got.off, want.offsets)
    assert np.array_equal(got.idx, np.concatenate(want.detections, axis=1)) and got.pw.tobytes() == np.concatenate(want.det_pow).tobytes()
    assert got.res.num_dets == want.numDets == got.res.n_rng and got.res.n_azi == 0
    assert got.rngEst.tobytes() == want.rngEst.tobytes() and got.velEst.tobytes() == want.velEst.tobytes()
    return got


METHOD_CASES = [("CA", 1, 0.0), ("GOCA", 1, 0.0), ("SOCA", 1, 0.0), ("OS", 1, 0.0), ("OS", 18, 0.0), ("OS", 24, 0.0), ("SOCA", 1, 20.0)]


def _method_cases(name):
    """METHOD_CASES at the scene's N: the OS ranks 1, 3N/4 and N (18 and 24 of the default 24 cells)."""
    n = M.n_train(*R.bands_of(name))
    return [(m, {18: 3 * n // 4, 24: n}.get(k, k) if m == "OS" else k, c) for m, k, c in METHOD_CASES]


@pytest.mark.parametrize("name", list(R.SCENES))
def test_redetect_equals_the_restatement_on_the_devices_own_window(pkg, ctx, name):
    r = _run(pkg, ctx, name)
    _again(pkg, ctx, r)
    seen = 0
    assert _method_cases("a4_273prb") == METHOD_CASES
    if name == R.BAND_SCENE:                                                   # hr != hc, gr != gc, and a window cut accordingly
        (gr, gc), (tr, tc) = R.bands_of(name)
        assert gr != gc and gr + tr != gc + tc and M.n_train(*R.bands_of(name)) == 78
        assert r.dbg.power_window.shape[:2] == (r.rect[1] - r.rect[0] + 1 + 2 * (gr + tr), r.rect[3] - r.rect[2] + 1 + 2 * (gc + tc))
        assert (r.dbg.first_row, r.dbg.first_col) == (r.rect[0] - gr - tr, r.rect[2] - gc - tc)
    for method, rank, custom in _method_cases(name):
        got = _check_against_restatement(pkg, ctx, r, method, rank, custom)
        seen += got.n_total
        print(f"{name} {method} rank {rank} custom {custom}: {got.n_total} detections, numDets {got.res.num_dets}")
        if method == "CA":                                                     # the lists of the fft2D call itself, byte for byte
            assert got.idx.tobytes() == np.concatenate(r.dbg.detections, axis=1).astype(np.int32).tobytes()
            assert got.pw.tobytes() == np.concatenate(r.dbg.det_pow).tobytes() and got.n_total >= 1
            assert got.rngEst.tobytes() == r.est.rngEst.tobytes() and got.velEst.tobytes() == r.est.velEst.tobytes()
    assert seen > 0


def _zone_around_strongest(r, n_rows=None, one_column=False):
    row0, row1, col0, col1 = r.rect
    a = int(np.argmax([p.max() if p.size else -1.0 for p in r.dbg.det_pow]))
    k = int(np.argmax(r.dbg.det_pow[a]))
    dr, dc = int(r.dbg.detections[a][0, k]), int(r.dbg.detections[a][1, k])
    if n_rows is not None:
        lo = min(max(row0, dr - n_rows // 2), row1 - n_rows + 1)
        assert lo >= row0
        row0, row1 = lo, lo + n_rows - 1
    if one_column:
        col0 = col1 = dc
    return (row0, row1, col0, col1)


def test_single_column_zone_and_a_row_count_one_past_the_panel_height(pkg, ctx):
    for name, kw in (("a4_24prb_generic", dict(one_column=True)), ("a4_24prb_generic", dict(n_rows=PANEL_ROWS + 1)), ("a4_273prb", dict(n_rows=2 * PANEL_ROWS + 1, one_column=True))):
        rect = _zone_around_strongest(_run(pkg, ctx, name), **kw)
        r = _run(pkg, ctx, name, rect)
        _again(pkg, ctx, r)
        assert r.rect == rect and r.dbg.power_window.shape[:2] == (rect[1] - rect[0] + 7, rect[3] - rect[2] + 7)
        n = sum(_check_against_restatement(pkg, ctx, r, m, k, c).n_total for m, k, c in METHOD_CASES)
        print(f"{name} zone {rect}: {n} detections over the method cases")
        assert n > 0


def test_chain_equals_the_oracle_only_result(pkg, ctx):
    """Scene -> device echo -> fft2D -> redetect against oracle echo -> oracle |rdm|^2 -> restatement, for the pairs whose thresholds clear the guard band."""
    cleared, dropped = M.chain_pairs()
    assert len(dropped) <= 1 and len(cleared) >= len(R.SCENES) * len(M.CHAIN_METHODS) - 1
    last = None
    for name, method, rank in cleared:
        r = _run(pkg, ctx, name)
        if last != name:
            _again(pkg, ctx, r)
            last = name
        want = M.oracle_redetect(name, method, rank)
        st, got = _redetect_raw(pkg, ctx, r.sc.A, method, rank)
        assert st == 0 and got.n_total == want.totalDetections and np.array_equal(got.off, want.offsets), (name, method)
        assert np.array_equal(got.idx, np.concatenate(want.detections, axis=1)), (name, method)
        assert np.array_equal(got.rngEst, want.rngEst) and np.array_equal(got.velEst, want.velEst) and got.res.num_dets == want.numDets
        wp = np.concatenate(want.det_pow)
        assert (np.abs(got.pw - wp) <= 1e-10 * wp).all()


def test_everything_else_is_untouched(pkg, ctx):
    """Power window, covariance, MUSIC spectrum, fft2D's own detection lists and the target list: byte-identical before and after re-detections."""
    r = _run(pkg, ctx, "a4_273prb")
    _again(pkg, ctx, r)
    F = _fft2d_mod(pkg)
    before, tl0 = F.fft2D_debug(ctx, r.sc.A), pkg.sensing.estimation.targetList(ctx, snapshots=True)
    for method, rank, custom in METHOD_CASES:
        assert _redetect_raw(pkg, ctx, r.sc.A, method, rank, custom)[0] == 0
    after, tl1 = F.fft2D_debug(ctx, r.sc.A), pkg.sensing.estimation.targetList(ctx, snapshots=True)
    for k in ("power_window", "Ra", "spectrum_db"):
        assert getattr(before, k).tobytes() == getattr(after, k).tobytes() == getattr(r.dbg, k).tobytes(), k
    for a, b in zip(before.detections + before.det_pow, after.detections + after.det_pow):
        assert a.tobytes() == b.tobytes()
    assert tl0.keys() == tl1.keys() and all(np.asarray(tl0[k]).tobytes() == np.asarray(tl1[k]).tobytes() for k in tl0)


def test_contract(pkg):
    L = pkg._lib
    sc = R.make("a4_24prb_generic")
    rp, cf = _blocks(pkg, sc)
    F = _fft2d_mod(pkg)
    c = pkg.Context()
    try:
        assert _redetect_raw(pkg, c, sc.A, "SOCA")[0] == INVALID_ARG              # before any fft2D
        d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
        echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c)
        est0 = pkg.sensing.estimation.fft2D(rp, cf, echo, d_txg, ctx=c)
        st, full = _redetect_raw(pkg, c, sc.A, "OS", 18)
        assert st == 0 and full.n_total > 2
        # bad arguments; capacity (n_total is set)
        for method, rank, custom in ((9, 1, 0.0), ("OS", 0, 0.0), ("OS", 25, 0.0), ("GOCA", 1, -2.0), ("GOCA", 1, float("nan"))):
            assert _redetect_raw(pkg, c, sc.A, method, rank, custom)[0] == INVALID_ARG
        m, res, n_total = L.CfarMethod(3, 18, 0.0), L.EstResult(), C.c_int32(-1)
        idx = np.zeros((2, 2), dtype=np.int32, order="F")
        assert c.lib.isac_fft2d_redetect(c.handle, C.byref(m), C.byref(res), idx.ctypes.data_as(C.c_void_p), None, 2, None, C.byref(n_total)) == CAPACITY
        assert n_total.value == full.n_total
        assert c.lib.isac_fft2d_redetect(c.handle, None, C.byref(res), None, None, 1 << 30, None, None) == INVALID_ARG
        # zero detections: ISAC_OK with empty lists
        st, none = _redetect_raw(pkg, c, sc.A, "GOCA", 1, 1e30)
        assert st == 0 and none.n_total == 0 and none.res.num_dets == 0 and none.res.n_rng == 0 and none.res.n_vel == 0 and not none.off.any()
        # a pending submit and its result survive a (refused) call in between
        F.fft2D_submit(rp, cf, echo, d_txg, ctx=c)
        assert _redetect_raw(pkg, c, sc.A, "SOCA")[0] == INVALID_ARG              # submitted, not collected: no completed fft2D
        est1 = F.fft2D_collect(c)
        for k in ("rngEst", "velEst", "aziEst"):
            assert getattr(est1, k).tobytes() == getattr(est0, k).tobytes(), k
        st, again = _redetect_raw(pkg, c, sc.A, "OS", 18)
        assert st == 0 and again.idx.tobytes() == full.idx.tobytes() and again.pw.tobytes() == full.pw.tobytes()
        # the range stage alone on OTHER grids rewrites the state the validity covers: no stale answer
        ep, cfb = import_module(pkg.__name__ + ".sensing._marshal").est_block(rp), F._cfar_block(cf)
        other = c.to_device(np.asfortranarray(sc.tx_grid[:, ::-1, :]))
        c.check(c.lib.isac_fft2d_range_stage_dev(c.handle, C.byref(ep), C.byref(cfb), other, d_txg, sc.K, sc.L, sc.A))
        assert _redetect_raw(pkg, c, sc.A, "SOCA")[0] == INVALID_ARG
        # a UPA: fft2D refuses the DoA after the range / velocity stages; the re-detection computes no direction and is accepted
        rp_upa = SimpleNamespace(**vars(rp))
        rp_upa.antennaType = SimpleNamespace(kind="upa", nV=2, nH=2)
        with pytest.raises(pkg.IsacError) as e:
            pkg.sensing.estimation.fft2D(rp_upa, cf, echo, d_txg, ctx=c)
        assert e.value.name == "UNSUPPORTED"
        st, upa = _redetect_raw(pkg, c, sc.A, "OS", 18)
        assert st == 0 and upa.idx.tobytes() == full.idx.tobytes() and upa.rngEst.tobytes() == full.rngEst.tobytes()
    finally:
        c.close()


def test_python_redetect_end_to_end(pkg, ctx):
    """sensing.estimation.redetect: rngEst / velEst of the C call, aziEst of the music mirror called by hand with the new numDets and the context's Ra."""
    r = _run(pkg, ctx, "a8_273prb")
    _again(pkg, ctx, r)
    st, raw = _redetect_raw(pkg, ctx, r.sc.A, "SOCA")
    est, dbg = pkg.sensing.estimation.redetect(ctx, Method="SOCA", return_debug=True)
    assert st == 0 and dbg.numDets == raw.res.num_dets >= 1 and dbg.numDets != len(r.est.rngEst)      # a model order fft2D's CA did not give
    assert est.rngEst.tobytes() == raw.rngEst.tobytes() and est.velEst.tobytes() == raw.velEst.tobytes()
    assert np.array_equal(np.concatenate(dbg.detections, axis=1), raw.idx) and dbg.Ra.tobytes() == r.dbg.Ra.tobytes()
    _, azi, ele = pkg.sensing.estimation.doaEstimation.music(dbg.numDets, r.rp, r.dbg.Ra, ctx=ctx)
    assert est.aziEst.tobytes() == azi.tobytes() and est.aziEst.size >= 1 and np.isnan(est.eleEst).all() and est.eleEst.size == ele.size
    ca = pkg.sensing.estimation.redetect(ctx)                                  # Method 'CA', 'Auto': fft2D's own answer
    for k in ("rngEst", "velEst", "aziEst"):
        assert getattr(ca, k).tobytes() == getattr(r.est, k).tobytes(), k
    os_c = pkg.sensing.estimation.redetect(ctx, Method="OS", Rank=18, ThresholdFactor="Custom", CustomThresholdFactor=_alpha(pkg, "OS", 24, float(r.rp.Pfa), 18))
    os_a = pkg.sensing.estimation.redetect(ctx, Method="OS", Rank=18)
    assert os_c.rngEst.tobytes() == os_a.rngEst.tobytes() and os_c.aziEst.tobytes() == os_a.aziEst.tobytes()
