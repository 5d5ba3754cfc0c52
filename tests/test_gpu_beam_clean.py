"""isac_fft2d_beam_clean_targets on the MI355X: successive target cancellation with the detector on beam planes of the last fft2D (project-defined --
include/isac_beam_clean.h).

Cases, scenes, beam sets and the oracle-only result come from tests/_beam_clean_restatement.py; tests/test_beam_clean_cpu.py has shown on the oracle that every decision of
every pass clears its margin by 1e-6 or more (the measured minimum is 8.5e-5), so nothing here is left out or skipped.  Each scene runs fft2D once per module and all its
cases behind it.  One refusal is not provoked here: nr nc n_beams >= 2^31 (tests/test_gpu_beam_detect.py says why no completed fft2D can leave such a window)."""
from __future__ import annotations

import ctypes as C
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import make_scene

import _beam_clean_restatement as BC
import _beam_detect_restatement as B
import _clean_restatement as K
import _target_list_restatement as T
import _target_list_upa_restatement as TU

pytestmark = pytest.mark.gpu

NU_TOL = 1e-6          # |nu_dev - nu_ref| L                    (tests/test_gpu_clean.py)
FIELD_TOL = 1e-10      # the project's field tolerance
INVALID_ARG, UNSUPPORTED = 1, 7
COUNTS = ("n_iter", "n_kept", "n_left")
INT_KEYS, F64_KEYS = ("row", "col", "hits", "beam", "status", "parent"), ("map_power", "nu", "vel", "rng", "power", "azi", "ele", "beam_label")
BIG_KEYS = ("snapshots", "residual", "beam_pow", "left_cells")
NEVER = dict(factor=1e300)   # a custom threshold factor no cell exceeds: the call returns the copy of the range rows untouched


def _blocks(pkg, sc):
    rp = pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)
    return rp, pkg.sensing.detection.cfar2D(rp)


def _dims(c):
    d = (C.c_int32 * 3)()
    c.check(c.lib.isac_fft2d_get_power_window(c.handle, None, 0, d, None, None))
    return int(d[0]), int(d[1]), int(d[2])


def _raw(pkg, c, L, W, dims=None, beam_azi=None, n_beams=None, max_iter=BC.MAX_ITER, span_rows=2, merge_tol=0.5, method="CA", rank=1, factor=None, sym_active=None, null=(),
         cap=None):
    """The C call itself: (status code, namespace of the raw outputs, every one pre-filled with a sentinel).  ``null``: the arguments passed as NULL; ``dims``: (nr, nc, A)
    when the context holds no CPI to ask."""
    nr, nc, A = dims if dims is not None else _dims(c)
    m = import_module(pkg.__name__ + ".sensing.detection.cfarDetect").method_block(method, rank, "Auto" if factor is None else "Custom", factor)
    w = np.asfortranarray(np.asarray(W, dtype=np.complex128))
    nb = w.shape[1] if n_beams is None else n_beams
    cap = max(max_iter, 1) if cap is None else cap
    o = SimpleNamespace(**{k: np.full(cap, -7, dtype=np.int32) for k in INT_KEYS}, **{k: np.full(cap, np.nan) for k in F64_KEYS},
                        snapshots=np.zeros((A, cap), dtype=np.complex128, order="F"), residual=np.zeros((nr, L, A), dtype=np.complex128, order="F"),
                        beam_pow=np.zeros((nr, nc, w.shape[1]), dtype=np.float64, order="F"), left_cells=np.full((pkg._lib.ISAC_MAX_TARGETS, 2), -7, dtype=np.int32))
    act = None if sym_active is None else np.ascontiguousarray(sym_active, dtype=np.uint8)
    lab = None if beam_azi is None else np.ascontiguousarray(beam_azi, dtype=np.float64)
    cnt = {k: C.c_int32(-7) for k in COUNTS}
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)              # noqa: E731
    p = lambda k: None if k in null else ptr(getattr(o, k))                          # noqa: E731
    q = lambda k: None if k in null else C.byref(cnt[k])                             # noqa: E731
    st = c.lib.isac_fft2d_beam_clean_targets(c.handle, None if "W" in null else ptr(w), nb, ptr(lab), None if "m" in null else C.byref(m), max_iter, span_rows, merge_tol, ptr(act),
                                             *(q(k) for k in COUNTS), *(p(k) for k in INT_KEYS), *(p(k) for k in F64_KEYS), *(p(k) for k in BIG_KEYS))
    for k, v in cnt.items():
        setattr(o, k, int(v.value))
    return st, o


def _untouched(o):
    """Every output of a refused call still holds its sentinel."""
    return (all(getattr(o, k) == -7 for k in COUNTS) and all((getattr(o, k) == -7).all() for k in INT_KEYS + ("left_cells",)) and
            all(np.isnan(getattr(o, k)).all() for k in F64_KEYS) and not o.snapshots.any() and not o.residual.any() and not o.beam_pow.any())


def _same_outputs(a, b):
    return all(getattr(a, k) == getattr(b, k) for k in COUNTS) and all(getattr(a, k).tobytes(order="A") == getattr(b, k).tobytes(order="A") for k in INT_KEYS + F64_KEYS + BIG_KEYS)


def _lists(pkg, c, upa, W):
    """What the other getters of the CPI return: the list, cleanTargets, beamDetect with its planes, the complex window."""
    est = pkg.sensing.estimation
    res, dbg = est.beamDetect(c, W, return_debug=True)
    Y, fr, fc = est.rdmWindow(c)
    return {"tl": (est.targetListUPA if upa else est.targetList)(c, snapshots=True), "clean": est.cleanTargets(c, snapshots=True, residual=True), "beam": res,
            "beam_pow": dbg.beam_pow, "beam_dets": {f"d{b}": v for b, v in enumerate(dbg.detections)}, "Y": Y, "first": (fr, fc)}


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], dict):
            _same(a[k], b[k])
        elif isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].tobytes(order="A") == b[k].tobytes(order="A"), k
        else:
            assert a[k] == b[k], k


_runs = {}


@pytest.fixture(scope="module")
def runs(pkg):
    """scene -> its run, made on first use: a context of its own, monoStaticSensing -> fft2D once, the other getters, every case of the scene (the C call) and the first of
    them a second time, the rows as they were (a call that detects nothing), sensing.estimation.beamClean, the other getters again.  Host copies only are kept."""
    def get(scene):
        if scene not in _runs:
            sc = BC.make(scene)
            rp, cf = _blocks(pkg, sc)
            cf = T.with_bands(scene, cf)                                     # the default bands for every scene but T.BAND_SCENE
            est_mod = pkg.sensing.estimation
            c = pkg.Context()
            c.set_upa_doa(True)
            try:
                d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
                echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c)
                est_mod.fft2D(rp, cf, echo, d_txg, ctx=c)
                g = BC.oracle_rows(scene).g
                cases = [k for k, v in BC.CASES.items() if v[0] == scene]
                W0, azi0 = BC.weights(scene, BC.CASES[cases[0]][1])
                before = _lists(pkg, c, BC.is_upa(scene), W0)
                raw, planes = {}, {}
                for case in cases:
                    W, azi = BC.weights(scene, BC.CASES[case][1])
                    kw = BC.keywords(case, g)
                    st, raw[case] = _raw(pkg, c, sc.L, W, beam_azi=azi, **kw)
                    assert st == 0, (case, c.last_error() if hasattr(c, "last_error") else st)
                    if BC.CASES[case][1] not in planes:                      # isac_fft2d_beam_detect's planes of the same context and weights
                        planes[BC.CASES[case][1]] = est_mod.beamDetect(c, W, return_debug=True)[1].beam_pow
                st, again = _raw(pkg, c, sc.L, W0, beam_azi=azi0, **BC.keywords(cases[0], g))
                assert st == 0
                st, rows0 = _raw(pkg, c, sc.L, W0, **NEVER)
                assert st == 0 and (rows0.n_iter, rows0.n_kept, rows0.n_left) == (0, 0, 0)
                kw0 = BC.keywords(cases[0], g)
                py = est_mod.beamClean(c, W0, beam_azi=azi0, maxIter=kw0.get("max_iter", BC.MAX_ITER), spanRows=kw0.get("span_rows", 2), mergeTol=kw0.get("merge_tol", 0.5),
                                       Method=kw0.get("method", "CA"), Rank=kw0.get("rank", 1), symActive=kw0.get("sym_active"), snapshots=True, residual=True, beamPow=True)
                after = _lists(pkg, c, BC.is_upa(scene), W0)
                for d in (echo, d_txg, d_wave):
                    d.free()
            finally:
                c.close()
            _runs[scene] = SimpleNamespace(sc=sc, rp=rp, cf=cf, g=g, cases=cases, raw=raw, planes=planes, again=again, rows0=rows0, py=py, before=before, after=after)
        return _runs[scene]

    yield get
    _runs.clear()


def _case(runs, case):
    scene, beams, _ = BC.CASES[case]
    r = runs(scene)
    return r, r.raw[case], BC.oracle_rows(scene), BC.oracle_beam_clean(case), BC.keywords(case, r.g), BC.weights(scene, beams)


def _cells(o, n):
    return list(zip(o.row[:n].tolist(), o.col[:n].tolist()))


@pytest.mark.parametrize("case", list(BC.CASES))
def test_decisions_equal_the_restatement(runs, case):
    """n_iter, n_kept, n_left, the cells, hits, beam, status, parent and left_cells of the device equal the restatement's on the oracle's range rows, exactly; what lies
    behind n_iter entries and behind the listed pairs is not written."""
    r, raw, s, want, _, _ = _case(runs, case)
    n = want.n_iter
    print(f"{case}: cells {_cells(raw, raw.n_iter)} beam {raw.beam[:raw.n_iter].tolist()} hits {raw.hits[:raw.n_iter].tolist()} parent {raw.parent[:raw.n_iter].tolist()} n_left {raw.n_left}")
    assert (raw.n_iter, raw.n_kept, raw.n_left) == (want.n_iter, want.n_kept, want.n_left)
    for k in INT_KEYS:
        assert np.array_equal(getattr(raw, k)[:n], getattr(want, k)), k
        assert (getattr(raw, k)[n:] == -7).all(), k
    assert np.array_equal(raw.left_cells[:want.n_left], want.left_cells) and (raw.left_cells[want.n_left:] == -7).all()


@pytest.mark.parametrize("case", list(BC.CASES))
def test_values_against_the_restatement(runs, case):
    """|nu_dev - nu_ref| L <= 1e-6 against the long-double bisection; power, map_power within 1e-10 relative and beam_pow within 1e-10 of each plane's maximum; vel = nu nFFT
    vRes, rng = (row - 1) rRes, beam_label = the label of the beam."""
    r, raw, s, want, _, (W, azi) = _case(runs, case)
    n = want.n_iter
    e_nu = np.abs(raw.nu[:n] - want.nu).max() * s.L
    e_p, e_s = np.abs(raw.power[:n] / want.power - 1).max(), np.abs(raw.map_power[:n] / want.map_power - 1).max()
    e_b = (np.abs(raw.beam_pow - want.beam_pow).max(axis=(0, 1)) / want.beam_pow.max(axis=(0, 1))).max()
    print(f"{case}: nu error {e_nu:.3e} / L, power error {e_p:.3e}, map power error {e_s:.3e} relative, beam planes {e_b:.3e} of the plane maximum")
    assert e_nu <= NU_TOL
    assert e_p <= FIELD_TOL and e_s <= FIELD_TOL and e_b <= FIELD_TOL
    assert np.array_equal(raw.vel[:n], raw.nu[:n] * s.g.n_fft * float(r.rp.vRes)) and np.array_equal(raw.rng[:n], (raw.row[:n] - 1) * float(r.rp.rRes))
    assert np.array_equal(raw.beam_label[:n], azi[raw.beam[:n] - 1]) and raw.beam[:n].min() >= 1 and raw.beam[:n].max() <= W.shape[1]


@pytest.mark.parametrize("case", list(BC.CASES))
def test_snapshots_and_direction(runs, case):
    """azi (and ele) = the lists' restatement of the Bartlett scan on the device's own snapshots, exactly; the snapshots within 1e-6 of max |x| of the restatement's."""
    r, raw, s, want, _, _ = _case(runs, case)
    n = want.n_iter
    x = raw.snapshots[:, :n]
    err = np.abs(x - want.snapshots).max() / np.abs(want.snapshots).max()
    print(f"{case}: snapshot error {err:.3e} of max |x|")
    assert err <= 1e-6
    if BC.is_upa(BC.CASES[case][0]):
        _, azi, ele, _, _ = TU.bartlett2d(x, r.sc.cell.gNBSenAntenna.nV, r.sc.cell.gNBSenAntenna.nH, r.rp)
        assert np.array_equal(raw.azi[:n], azi) and np.array_equal(raw.ele[:n], ele)
    else:
        _, azi, _, _ = T.bartlett(x, r.rp)
        assert np.array_equal(raw.azi[:n], azi) and np.isnan(raw.ele).all()  # a ULA: ele is not written


@pytest.mark.parametrize("case", list(BC.CASES))
def test_residual_rows_against_the_long_double_replay(runs, case):
    """The rows a call that detects nothing returns are the device's range rows (the oracle's to 1e-10 of their maximum); from them, step 7 replayed in long double at the
    device's own (row, nu) sequence gives residual_rows within 16 L 2^-53 max |y|; rows outside every span keep their bytes."""
    r, raw, s, want, kw, _ = _case(runs, case)
    n, span, rows0 = raw.n_iter, kw.get("span_rows", 2), r.rows0.residual
    assert rows0.shape == s.rows.shape and np.abs(rows0 - s.rows).max() <= FIELD_TOL * np.abs(s.rows).max()
    ref = K.replay(rows0, s.g, raw.row[:n], raw.nu[:n], span, kw.get("sym_active"))
    bound = 16 * s.L * 2.0 ** -53 * np.abs(rows0).max()
    err = float(np.abs(raw.residual.astype(np.clongdouble) - ref).max())
    print(f"{case}: residual error {err:.3e} against the bound {bound:.3e} ({err / bound:.3e} of it)")
    assert err <= bound
    touched = BC.touched_rows(raw_view(raw, n), s.g, span)
    rest = np.setdiff1d(np.arange(s.g.n_rows), touched)
    assert len(touched) >= 1 and raw.residual[rest].tobytes() == rows0[rest].tobytes()
    assert np.abs(raw.residual[touched] - rows0[touched]).max() > 0


def raw_view(raw, n):
    return SimpleNamespace(row=raw.row[:n], status=raw.status[:n])


@pytest.mark.parametrize("case", list(BC.CASES))
def test_band_update_leaves_no_stale_row(runs, case):
    """The planes the last pass saw: the rows outside every touched band equal, byte for byte, the beam_pow isac_fft2d_beam_detect returns on the same context with the same
    weights (they were formed once, in pass 0); every row -- the touched ones included -- matches the restatement's planes of the device's own residual_rows to 1e-10 of
    the plane maximum.  The pass-0 planes of a call that detects nothing are isac_fft2d_beam_detect's, whole."""
    r, raw, s, want, kw, (W, _) = _case(runs, case)
    n, span = raw.n_iter, kw.get("span_rows", 2)
    full = r.planes[BC.CASES[case][1]]
    touched = BC.touched_rows(raw_view(raw, n), s.g, span)
    rest = np.setdiff1d(np.arange(s.g.n_rows), touched)
    assert full.shape == raw.beam_pow.shape and raw.beam_pow[rest].tobytes() == full[rest].tobytes()
    assert len(touched) >= 1 and np.abs(raw.beam_pow[touched] - full[touched]).max() > 0
    ref = BC.planes_of_rows(raw.residual, s.g, W)
    err = (np.abs(raw.beam_pow - ref).max(axis=(0, 1)) / ref.max(axis=(0, 1))).max()
    err_in = (np.abs(raw.beam_pow[touched] - ref[touched]).max(axis=(0, 1)) / ref.max(axis=(0, 1))).max()
    print(f"{case}: {len(touched)} touched rows of {s.g.n_rows}; planes of the residual rows: error {err:.3e} of the plane maximum ({err_in:.3e} inside the bands)")
    assert err <= FIELD_TOL
    # ... and the decisions of the closing pass are the restatement's steps 2-3 on the device's own planes: a stale flag or a stale M / b* / hits shows here
    t = BC.cells_of_planes(raw.beam_pow, s.g, kw.get("method", "CA"), kw.get("rank", 1))
    assert t.row.size == raw.n_left and np.array_equal(np.stack([t.row, t.col], axis=1).reshape(-1, 2), raw.left_cells[:raw.n_left])


@pytest.mark.parametrize("scene", list(BC.SCENES))
def test_repeat_python_dict_and_untouched_getters(pkg, runs, scene):
    """A repeat call gives identical bytes; a call that detects nothing returns isac_fft2d_beam_detect's planes; sensing.estimation.beamClean returns the kept entries of
    the C call, which getRMSE, refineTargets, relaxTargets and resolveDirections take; targetList, cleanTargets, beamDetect and rdmWindow return after the calls the bytes
    they returned before them."""
    r = runs(scene)
    _same(r.before, r.after)
    case = r.cases[0]
    raw, d = r.raw[case], r.py
    assert _same_outputs(raw, r.again)
    assert r.rows0.beam_pow.tobytes(order="F") == r.before["beam_pow"].tobytes(order="F")
    n = raw.n_iter
    kept = np.flatnonzero(raw.parent[:n] == np.arange(n))
    assert d["n_total"] == n and d["n_left"] == raw.n_left and d["row"].size == raw.n_kept == kept.size
    for k in ("row", "col", "hits", "beam", "status", "map_power", "nu", "vel", "rng", "power", "azi", "beam_label"):
        assert d[k].tobytes() == getattr(raw, k)[:n][kept].tobytes(), k
    assert d["parent"].tolist() == list(range(kept.size)) and d["n_merged"].tolist() == np.bincount(raw.parent[:n], minlength=n)[kept].tolist()
    assert ("ele" in d) == BC.is_upa(scene) and (not BC.is_upa(scene) or d["ele"].tobytes() == raw.ele[:n][kept].tobytes())
    assert d["snapshots"].tobytes(order="F") == np.asfortranarray(raw.snapshots[:, :n][:, kept]).tobytes(order="F")
    assert d["residual"].tobytes(order="F") == raw.residual.tobytes(order="F") and d["beam_pow"].tobytes(order="F") == raw.beam_pow.tobytes(order="F")
    assert np.array_equal(d["left_cells"], raw.left_cells[:raw.n_left])
    rm = pkg.sensing.postProcessing.getRMSE(d, r.rp)
    assert rm.velRMSE.size == kept.size and np.isfinite(rm.rngRMSE[0]) and np.isfinite(rm.velRMSE[0])   # (an entry within no resolution cell of a true target has no error: NaN)


def test_the_other_calls_take_the_result(pkg):
    """refineTargets, relaxTargets and resolveDirections take beamClean's dict as they take cleanTargets'."""
    sc = BC.make("a4_24prb_generic")
    rp, cf = _blocks(pkg, sc)
    W, azi = BC.weights("a4_24prb_generic", "b5")
    est_mod = pkg.sensing.estimation
    c = pkg.Context()
    try:
        d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
        echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c)
        est_mod.fft2D(rp, cf, echo, d_txg, ctx=c)
        d = est_mod.beamClean(c, W, beam_azi=azi, snapshots=True)
        k = est_mod.cleanTargets(c, snapshots=True)
        assert d["row"].size == 2
        for call in (lambda x: est_mod.refineTargets(c, x), lambda x: est_mod.relaxTargets(c, x), lambda x: est_mod.resolveDirections(c, rp, x)):
            a, b = call(d), call(k)
            assert type(a) is type(b) and (not isinstance(a, dict) or a.keys() == b.keys())
    finally:
        c.close()


def test_capability_a_weak_target_under_the_sidelobes_needs_both(pkg, runs):
    """The 8-element scene with the second echo 30 dB down: cleanTargets (no array gain) and beamDetect (one map) do not list the weak target's cell (88, 124); beamClean
    returns exactly [(88, 134), (88, 124)] with n_left = 0, and its second velocity is closer to the truth than any beamDetect entry."""
    r = runs(BC.CAP)
    d, cl, bd = r.py, r.before["clean"], r.before["beam"]
    weak = BC.CAP_CELLS[1]
    assert weak not in list(zip(cl["row"].tolist(), cl["col"].tolist())) and weak not in list(zip(bd["row"].tolist(), bd["col"].tolist()))
    assert list(zip(d["row"].tolist(), d["col"].tolist())) == BC.CAP_CELLS and d["n_left"] == 0 and d["left_cells"].shape == (0, 2)
    truth = BC.true_velocity(r.rp, 1)
    print(f"truth {truth:.4f} m/s: beamClean {d['vel'][1]:.4f} on beam {d['beam'][1]}, beamDetect {bd['vel'].round(4).tolist()}, cleanTargets cells {list(zip(cl['row'].tolist(), cl['col'].tolist()))}")
    assert abs(d["vel"][1] - truth) < np.abs(bd["vel"] - truth).min()


def test_a_pending_submit_is_unharmed(pkg, runs):
    """Submitted, not collected: the call is refused and writes nothing; the collected CPI then gives the estimates and the answer of an undisturbed context."""
    r = runs("a4_24prb_generic")
    sc, case = r.sc, r.cases[0]
    W, azi = BC.weights("a4_24prb_generic", BC.CASES[case][1])
    F = import_module(pkg.__name__ + ".sensing.estimation.fft2D")
    c, ref = pkg.Context(), pkg.Context()
    try:
        d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
        echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, r.rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c)
        r_txg, r_wave = ref.to_device(sc.tx_grid), ref.to_device(sc.tx_wave)
        r_echo = pkg.sensing.monoStaticSensing(r_wave, sc.tx_grid.shape, sc.carrier, r.rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=ref)
        est_ref = pkg.sensing.estimation.fft2D(r.rp, r.cf, r_echo, r_txg, ctx=ref)
        F.fft2D_submit(r.rp, r.cf, echo, d_txg, ctx=c)
        st, o = _raw(pkg, c, sc.L, W, dims=(r.g.n_rows, r.raw[case].beam_pow.shape[1], sc.A), beam_azi=azi)
        assert st == INVALID_ARG and _untouched(o)
        est = F.fft2D_collect(c)
        for k in ("rngEst", "velEst", "aziEst"):
            assert getattr(est, k).tobytes() == getattr(est_ref, k).tobytes(), k
        st, o = _raw(pkg, c, sc.L, W, beam_azi=azi, **BC.keywords(case, r.g))
        assert st == 0 and _same_outputs(o, r.raw[case])
    finally:
        c.close()
        ref.close()


def test_contract(pkg):
    """ISAC_ERR_INVALID_ARG (1) before any fft2D, for n_beams < 1, max_iter outside 1 .. ISAC_MAX_TARGETS, a negative span, a negative or non-finite tolerance, a mask without
    an active symbol, every NULL required array, a weight column with a zero or non-finite norm, a bad detector block, a UPA without ele, and after the range stage has
    rewritten the rows; ISAC_ERR_UNSUPPORTED (7) for more than ISAC_MAX_BEAMS beams.  Every refused call leaves its outputs' sentinels, the CPI and the next answer alone."""
    L = pkg._lib
    scene = "upa2x4_24prb"
    sc = BC.make(scene)
    s = BC.oracle_rows(scene)
    rp, cf = _blocks(pkg, sc)
    W, azi = BC.weights(scene, "b5")
    est_mod = pkg.sensing.estimation
    c = pkg.Context()
    c.set_upa_doa(True)
    try:
        dims = (s.g.n_rows, s.g.rect[3] - s.g.rect[2] + 1 + 2 * s.g.hc, sc.A)
        st, o = _raw(pkg, c, sc.L, W, dims=dims)
        assert st == INVALID_ARG and _untouched(o)                            # before any fft2D
        d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
        echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c)
        est_mod.fft2D(rp, cf, echo, d_txg, ctx=c)
        assert _dims(c) == dims
        st, full = _raw(pkg, c, sc.L, W, beam_azi=azi)
        want = BC.oracle_beam_clean(scene)
        assert st == 0 and full.n_iter == want.n_iter and np.array_equal(full.row[:full.n_iter], want.row)

        def refused(code, **kw):
            st, o = _raw(pkg, c, sc.L, kw.pop("W", W), **kw)
            assert st == code and _untouched(o), kw

        for kw in (dict(n_beams=0), dict(n_beams=-1), dict(max_iter=0), dict(max_iter=-1), dict(max_iter=L.ISAC_MAX_TARGETS + 1, cap=1), dict(span_rows=-1), dict(merge_tol=-1.0),
                   dict(merge_tol=float("nan")), dict(merge_tol=float("inf")), dict(sym_active=np.zeros(sc.L))):
            refused(INVALID_ARG, **kw)
        for k in ("W", "m") + COUNTS + INT_KEYS + F64_KEYS:                   # ele: a planar array needs it
            refused(INVALID_ARG, null=(k,))
        for bad in (0.0, np.nan, np.inf):                                     # a column with a zero / non-finite norm
            Wb = W.copy()
            Wb[:, 3] = bad
            refused(INVALID_ARG, W=Wb)
        refused(INVALID_ARG, method="OS", rank=0)                             # the method block: the cases of isac_cfar2d
        refused(INVALID_ARG, method="OS", rank=25)
        refused(INVALID_ARG, factor=-1.0)
        refused(UNSUPPORTED, W=np.ones((sc.A, L.ISAC_MAX_BEAMS + 1), dtype=np.complex128))
        st, opt = _raw(pkg, c, sc.L, W, beam_azi=azi, null=BIG_KEYS)          # the four optional arrays
        assert st == 0 and opt.nu.tobytes() == full.nu.tobytes()
        st, nolab = _raw(pkg, c, sc.L, W)                                    # no labels: the beam number
        assert st == 0 and np.array_equal(nolab.beam_label[:nolab.n_iter], nolab.beam[:nolab.n_iter].astype(np.float64))
        st, big = _raw(pkg, c, sc.L, W, beam_azi=azi, max_iter=L.ISAC_MAX_TARGETS)   # ISAC_MAX_TARGETS itself is served
        assert st == 0 and big.n_iter == full.n_iter and big.nu[:big.n_iter].tobytes() == full.nu[:full.n_iter].tobytes()
        st, wide = _raw(pkg, c, sc.L, W, span_rows=2 ** 31 - 1)              # a span wider than the window: clipped to it
        assert st == 0 and wide.n_iter >= 1
        one = np.zeros(sc.L)
        one[3] = 1
        assert _raw(pkg, c, sc.L, W, sym_active=one)[0] == 0                 # one active symbol is enough
        with pytest.raises(pkg.IsacError) as e:
            est_mod.beamClean(c, W, mergeTol=-1)
        assert e.value.name == "INVALID_ARG"
        for bad in (dict(symActive=np.ones(sc.L + 1)), dict(residual=True, nSymbols=sc.L + 1), dict(beam_azi=np.zeros(4))):
            with pytest.raises(ValueError):
                est_mod.beamClean(c, W, **bad)
        with pytest.raises(ValueError):
            est_mod.beamClean(c, W[:-1])                                      # A - 1 rows
        none = est_mod.beamClean(c, W, CustomThresholdFactor=1e300, ThresholdFactor="Custom")
        assert "ele" in none and none["row"].size == 0 and none["left_cells"].shape == (0, 2)   # a planar array: the key is there with no entry at all
        st, again = _raw(pkg, c, sc.L, W, beam_azi=azi)                      # none of the refusals disturbed the CPI; the scratch is reused
        assert st == 0 and _same_outputs(again, full)
        # the range stage alone on OTHER grids rewrites the range rows: no stale answer
        im = import_module
        ep, cfb = im(pkg.__name__ + ".sensing._marshal").est_block(rp), im(pkg.__name__ + ".sensing.estimation.fft2D")._cfar_block(cf)
        other = c.to_device(np.asfortranarray(sc.tx_grid[:, ::-1, :]))
        c.check(c.lib.isac_fft2d_range_stage_dev(c.handle, C.byref(ep), C.byref(cfb), other, d_txg, sc.K, sc.L, sc.A))
        st, o = _raw(pkg, c, sc.L, W, dims=dims)
        assert st == INVALID_ARG and _untouched(o)
    finally:
        c.close()


def _completed(pkg, c, sc, rp, cf):
    d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
    echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c)
    try:
        pkg.sensing.estimation.fft2D(rp, cf, echo, d_txg, ctx=c)
    except pkg.IsacError as e:                                              # a CPI without a detection, or a planar array with ISAC_OPT_UPA_DOA off, is still a completed one
        if e.name not in ("NO_DETECTION", "UNSUPPORTED"):
            raise
    return echo, d_txg, d_wave


@pytest.mark.parametrize("guard,train", [((2, 0), (1, 0)), ((0, 2), (0, 1))])
def test_a_halo_of_zero_is_unsupported(pkg, guard, train):
    """guard + training = 0 in one dimension: fft2D completes, the window carries no neighbours there, the local-maximum test cannot be made."""
    sc = BC.make("a4_24prb_generic")
    rp, cf = _blocks(pkg, sc)
    cf.cfarDetector2D.GuardBandSize, cf.cfarDetector2D.TrainingBandSize = tuple(guard), tuple(train)
    W, _ = BC.weights("a4_24prb_generic", "b5")
    c = pkg.Context()
    try:
        keep = _completed(pkg, c, sc, rp, cf)
        st, o = _raw(pkg, c, sc.L, W)
        assert st == UNSUPPORTED and _untouched(o)
        with pytest.raises(pkg.IsacError) as e:
            pkg.sensing.estimation.beamClean(c, W)
        assert e.value.name == "UNSUPPORTED" and "isac_fft2d_beam_clean_targets" in str(e.value) and "halo" in str(e.value)
    finally:
        c.close()


def test_the_refinements_lds_refusal_is_the_calls(pkg):
    """nFFT = 16 against L = 112 symbols: the refinement's probe table does not fit the 160 KB of LDS (tests/test_gpu_clean.py); the call, which runs the same device code
    on its residual rows, refuses the CPI the same way, before any pass."""
    sc = make_scene(n_ants=4, n_slots=8, nrb=24, num_slots_param=1, seed=24, **T._TWO24)
    rp, cf = _blocks(pkg, sc)
    assert (int(rp.nFFT), sc.L) == (16, 112)
    W = pkg.sensing.estimation.beamWeights(rp, B.beam_set(sc, "b5")[0])
    c = pkg.Context()
    try:
        keep = _completed(pkg, c, sc, rp, cf)
        st, o = _raw(pkg, c, sc.L, W)
        assert st == UNSUPPORTED and _untouched(o)
        with pytest.raises(pkg.IsacError) as e:
            pkg.sensing.estimation.beamClean(c, W)
        assert e.value.name == "UNSUPPORTED" and "isac_fft2d_beam_clean_targets" in str(e.value) and "LDS" in str(e.value)
    finally:
        c.close()


def test_a_planar_array_of_more_than_256_elements_is_unsupported(pkg):
    """16 x 17 elements (A = 272) at 24 PRB: a completed fft2D of a planar array the 2-D scan does not serve.  The call refuses it before any pass and writes nothing."""
    sc = make_scene(n_ants=272, n_slots=2, nrb=24, num_slots_param=6, seed=48, **T._TWO24)
    sc.cell.gNBSenAntenna = SimpleNamespace(kind="upa", nV=16, nH=17, dV=0.5, dH=0.5)
    rp, cf = _blocks(pkg, sc)
    W = np.ones((272, 2), dtype=np.complex128)
    c = pkg.Context()
    try:
        keep = _completed(pkg, c, sc, rp, cf)
        assert _dims(c)[2] == 272                                           # the CPI is there
        st, o = _raw(pkg, c, sc.L, W)
        assert st == UNSUPPORTED and _untouched(o)
        with pytest.raises(pkg.IsacError) as e:
            pkg.sensing.estimation.beamClean(c, W)
        assert e.value.name == "UNSUPPORTED" and "256" in str(e.value)
    finally:
        c.close()
