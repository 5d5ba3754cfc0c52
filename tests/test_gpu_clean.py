"""isac_fft2d_clean_targets on the MI355X: successive target cancellation on the range rows of the last fft2D (project-defined -- include/isac_clean.h, DESIGN.md
section 5).

Cases, scenes and the oracle-only result come from tests/_clean_restatement.py; tests/test_clean_cpu.py has shown on the oracle that every decision of every pass clears
its margin by 1e-6 or more (the measured minimum is 3.3e-4), so nothing here is left out or skipped.  Each scene runs fft2D once per module and all its cases behind it."""
from __future__ import annotations

import ctypes as C
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import make_scene

import _clean_restatement as K
import _target_list_restatement as T
import _target_list_upa_restatement as TU

pytestmark = pytest.mark.gpu

NU_TOL = 1e-6          # |nu_dev - nu_ref| L
FIELD_TOL = 1e-10      # the project's field tolerance
INVALID_ARG, UNSUPPORTED = 1, 7
INT_KEYS, F64_KEYS = ("row", "col", "hits", "status", "parent"), ("map_power", "nu", "vel", "rng", "power", "azi", "ele")
NEVER = dict(factor=1e300)   # a custom threshold factor no cell exceeds: the call returns the copy of the range rows untouched


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context()
    c.set_upa_doa(True)
    yield c
    c.close()


def _blocks(pkg, sc):
    rp = pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)
    return rp, pkg.sensing.detection.cfar2D(rp)


def _dims(c):
    d = (C.c_int32 * 3)()
    c.check(c.lib.isac_fft2d_get_power_window(c.handle, None, 0, d, None, None))
    return int(d[0]), int(d[1]), int(d[2])


def _raw(pkg, c, L, dims=None, max_iter=K.MAX_ITER, span_rows=2, merge_tol=0.5, method="CA", rank=1, factor=None, sym_active=None, null=(), cap=None):
    """The C call itself: (status code, namespace of the raw outputs).  ``null``: the arguments passed as NULL; ``dims``: (nr, A) when the context holds no CPI to ask."""
    nr, A = dims if dims is not None else (_dims(c)[0], _dims(c)[2])
    m = import_module(pkg.__name__ + ".sensing.detection.cfarDetect").method_block(method, rank, "Auto" if factor is None else "Custom", factor)
    cap = max(max_iter, 1) if cap is None else cap
    o = SimpleNamespace(**{k: np.full(cap, -7, dtype=np.int32) for k in INT_KEYS}, **{k: np.full(cap, np.nan) for k in F64_KEYS},
                        snapshots=np.zeros((A, cap), dtype=np.complex128, order="F"), residual=np.zeros((nr, L, A), dtype=np.complex128, order="F"))
    act = None if sym_active is None else np.ascontiguousarray(sym_active, dtype=np.uint8)
    cnt = {k: C.c_int32(-7) for k in ("n_iter", "n_kept", "n_left")}
    p = lambda k: None if k in null else getattr(o, k).ctypes.data_as(C.c_void_p)    # noqa: E731
    q = lambda k: None if k in null else C.byref(cnt[k])                             # noqa: E731
    st = c.lib.isac_fft2d_clean_targets(c.handle, None if "m" in null else C.byref(m), max_iter, span_rows, merge_tol, None if act is None else act.ctypes.data_as(C.c_void_p),
                                        q("n_iter"), q("n_kept"), q("n_left"), *(p(k) for k in INT_KEYS), *(p(k) for k in F64_KEYS), p("snapshots"), p("residual"))
    for k, v in cnt.items():
        setattr(o, k, int(v.value))
    return st, o


def _lists(pkg, c, upa):
    """What the other getters of the CPI return: the list (with snapshots), its refinement, and -- a ULA -- the re-detection."""
    est = pkg.sensing.estimation
    tl = (est.targetListUPA if upa else est.targetList)(c, snapshots=True)
    out = {"tl": tl, "refine": est.refineTargets(c, tl, snapshots=True)}
    if not upa:
        e, d = est.redetect(c, Method="SOCA", return_debug=True)
        out["redetect"] = {**{k: np.asarray(v) for k, v in vars(e).items()}, **{f"det{a}": v for a, v in enumerate(d.detections)}, **{f"pow{a}": v for a, v in enumerate(d.det_pow)}}
    return out


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


def _scene(pkg, ctx, scene):
    """Scene through monoStaticSensing -> isac_fft2d_dev, then: the other getters, every case of the scene (the C call), the rows as they were (a call that detects
    nothing), sensing.estimation.cleanTargets, the other getters again.  Once per module (host copies only)."""
    if scene not in _runs:
        sc = K.make(scene)
        rp, cf = _blocks(pkg, sc)
        cf = T.with_bands(scene, cf)                                         # the default bands for every scene but K.BANDS_SCENE
        est_mod = pkg.sensing.estimation
        d_txg, d_wave = ctx.to_device(sc.tx_grid), ctx.to_device(sc.tx_wave)
        echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=ctx)
        est_mod.fft2D(rp, cf, echo, d_txg, ctx=ctx)
        before = _lists(pkg, ctx, K.is_upa(scene))
        raw = {}
        for case, (s, kw) in K.CASES.items():
            if s == scene:
                st, raw[case] = _raw(pkg, ctx, sc.L, **kw)
                assert st == 0, (case, ctx.last_error() if hasattr(ctx, "last_error") else st)
        st, rows0 = _raw(pkg, ctx, sc.L, **NEVER)
        assert st == 0 and (rows0.n_iter, rows0.n_kept, rows0.n_left) == (0, 0, 0)
        py = est_mod.cleanTargets(ctx, maxIter=K.MAX_ITER, snapshots=True, residual=True)   # (the symbol count: recorded on the context by fft2D)
        py_mask = est_mod.cleanTargets(ctx, maxIter=K.MAX_ITER, symActive=K.GAP_MASK, snapshots=True, residual=True, nSymbols=sc.L) if scene == "masked_gap" else None
        after = _lists(pkg, ctx, K.is_upa(scene))
        for d in (echo, d_txg, d_wave):
            d.free()
        _runs[scene] = SimpleNamespace(sc=sc, rp=rp, cf=cf, raw=raw, rows0=rows0.residual, py=py, py_mask=py_mask, before=before, after=after)
    return _runs[scene]


def _case(pkg, ctx, case):
    scene, kw = K.CASES[case]
    r = _scene(pkg, ctx, scene)
    return r, r.raw[case], K.oracle_rows(scene), K.oracle_clean(case), kw


@pytest.mark.parametrize("case", list(K.CASES))
def test_decisions_equal_the_restatement(pkg, ctx, case):
    """n_iter, n_kept, n_left, the cells, hits, status and parent of the device equal the restatement's on the oracle's range rows, exactly; what lies behind n_iter is
    not written."""
    r, raw, s, want, _ = _case(pkg, ctx, case)
    n = want.n_iter
    print(f"{case}: cells {list(zip(raw.row[:raw.n_iter].tolist(), raw.col[:raw.n_iter].tolist()))} hits {raw.hits[:raw.n_iter].tolist()} parent {raw.parent[:raw.n_iter].tolist()} "
          f"n_left {raw.n_left}")
    assert (raw.n_iter, raw.n_kept, raw.n_left) == (want.n_iter, want.n_kept, want.n_left)
    for k in INT_KEYS:
        assert np.array_equal(getattr(raw, k)[:n], getattr(want, k)), k
        assert (getattr(raw, k)[n:] == -7).all(), k


@pytest.mark.parametrize("case", list(K.CASES))
def test_values_against_the_restatement(pkg, ctx, case):
    """|nu_dev - nu_ref| L <= 1e-6 against the long-double bisection; power and map_power within 1e-10 relative; vel = nu nFFT vRes and rng = (row - 1) rRes."""
    r, raw, s, want, _ = _case(pkg, ctx, case)
    n = want.n_iter
    e_nu = np.abs(raw.nu[:n] - want.nu).max() * s.L
    e_p, e_s = np.abs(raw.power[:n] / want.power - 1).max(), np.abs(raw.map_power[:n] / want.map_power - 1).max()
    print(f"{case}: nu error {e_nu:.3e} / L, power error {e_p:.3e}, map power error {e_s:.3e} relative")
    assert e_nu <= NU_TOL
    assert e_p <= FIELD_TOL and e_s <= FIELD_TOL
    assert np.array_equal(raw.vel[:n], raw.nu[:n] * s.g.n_fft * float(r.rp.vRes)) and np.array_equal(raw.rng[:n], (raw.row[:n] - 1) * float(r.rp.rRes))


@pytest.mark.parametrize("case", list(K.CASES))
def test_snapshots_and_direction(pkg, ctx, case):
    """azi (and ele) = the lists' restatement of the Bartlett scan on the device's own snapshots, exactly; the snapshots within 1e-6 of max |x| of the restatement's (their
    nu differs by up to 1e-6 / L)."""
    r, raw, s, want, _ = _case(pkg, ctx, case)
    n = want.n_iter
    x = raw.snapshots[:, :n]
    err = np.abs(x - want.snapshots).max() / np.abs(want.snapshots).max()
    print(f"{case}: snapshot error {err:.3e} of max |x|")
    assert err <= 1e-6
    if K.is_upa(K.CASES[case][0]):
        _, azi, ele, _, _ = TU.bartlett2d(x, r.sc.nV, r.sc.nH, r.rp)
        assert np.array_equal(raw.azi[:n], azi) and np.array_equal(raw.ele[:n], ele)
    else:
        _, azi, _, _ = T.bartlett(x, r.rp)
        assert np.array_equal(raw.azi[:n], azi) and np.isnan(raw.ele).all()  # a ULA: ele is not written


@pytest.mark.parametrize("case", list(K.CASES))
def test_residual_rows_against_the_long_double_replay(pkg, ctx, case):
    """The rows a call that detects nothing returns are the device's range rows (the oracle's to 1e-10 of their maximum); from them, step 8 replayed in long double at the
    device's own (row, nu) sequence gives residual_rows within 16 L 2^-53 max |y|; rows outside every span keep their bytes."""
    r, raw, s, want, kw = _case(pkg, ctx, case)
    n, span = raw.n_iter, kw.get("span_rows", 2)
    assert r.rows0.shape == s.rows.shape and np.abs(r.rows0 - s.rows).max() <= FIELD_TOL * np.abs(s.rows).max()
    ref = K.replay(r.rows0, s.g, raw.row[:n], raw.nu[:n], span, kw.get("sym_active"))
    bound = 16 * s.L * 2.0 ** -53 * np.abs(r.rows0).max()
    err = float(np.abs(raw.residual.astype(np.clongdouble) - ref).max())
    print(f"{case}: residual error {err:.3e} against the bound {bound:.3e} ({err / bound:.3e} of it)")
    assert err <= bound
    touched = sorted({wr for row in raw.row[:n] for wr in K.span_of(row, s.g.first_row, s.g.n_rows, span)})
    rest = np.setdiff1d(np.arange(s.g.n_rows), touched)
    assert len(touched) >= 1 and raw.residual[rest].tobytes() == r.rows0[rest].tobytes()
    assert np.abs(raw.residual[touched] - r.rows0[touched]).max() > 0


@pytest.mark.parametrize("scene", list(K.SCENES))
def test_python_dict_and_untouched_getters(pkg, ctx, scene):
    """sensing.estimation.cleanTargets returns the kept entries of the C call with the defaults, which getRMSE takes; targetList, refineTargets and redetect return after
    the calls the bytes they returned before them."""
    r = _scene(pkg, ctx, scene)
    _same(r.before, r.after)
    raw, d = r.raw[scene if scene != "masked_gap" else "masked_gap_nomask"], r.py
    n = raw.n_iter
    kept = np.flatnonzero(raw.parent[:n] == np.arange(n))
    assert d["n_total"] == n and d["n_left"] == raw.n_left and d["row"].size == raw.n_kept == kept.size
    for k in ("row", "col", "hits", "status", "map_power", "nu", "vel", "rng", "power", "azi"):
        assert d[k].tobytes() == getattr(raw, k)[:n][kept].tobytes(), k
    assert d["parent"].tolist() == list(range(kept.size)) and d["n_merged"].tolist() == np.bincount(raw.parent[:n], minlength=n)[kept].tolist()
    assert ("ele" in d) == K.is_upa(scene) and (not K.is_upa(scene) or d["ele"].tobytes() == raw.ele[:n][kept].tobytes())
    assert d["snapshots"].tobytes(order="F") == np.asfortranarray(raw.snapshots[:, :n][:, kept]).tobytes(order="F") and d["residual"].tobytes(order="F") == raw.residual.tobytes(order="F")
    rm = pkg.sensing.postProcessing.getRMSE(d, r.rp)
    assert rm.velRMSE.size == kept.size and np.isfinite(rm.rngRMSE).all()


def test_masked_target_through_the_python_call(pkg, ctx):
    """The masked scene end to end: the weak target's cell is not in targetList's answer and is in cleanTargets'; its velocity error is smaller than that of any listed
    entry.  With the gap, symActive is what finds it."""
    r = _scene(pkg, ctx, "masked")
    tl, d = r.before["tl"], r.py
    cells = list(zip(d["row"].tolist(), d["col"].tolist()))
    assert K.MASKED_CELL not in list(zip(tl["row"].tolist(), tl["col"].tolist())) and cells[1] == K.MASKED_CELL and d["hits"][1] >= 1
    truth = K.true_velocity(r.rp, 1)
    print(f"truth {truth:.4f} m/s: cleanTargets {d['vel'][1]:.4f}, targetList {tl['vel'].round(4).tolist()}")
    assert abs(d["vel"][1] - truth) < np.abs(tl["vel"] - truth).min()
    g = _scene(pkg, ctx, "masked_gap")
    assert g.raw["masked_gap"].n_iter == 2 and g.raw["masked_gap_nomask"].n_iter == 1
    m, raw = g.py_mask, g.raw["masked_gap"]                                  # symActive through the Python call: the C call's answer with the same mask
    assert list(zip(m["row"].tolist(), m["col"].tolist())) == [(88, 134), K.MASKED_CELL] and m["n_left"] == 0 and g.py["row"].size == 1
    assert m["nu"].tobytes() == raw.nu[:2].tobytes() and m["residual"].tobytes(order="F") == raw.residual.tobytes(order="F")


def test_stored_and_lazy_grid_give_the_same_bytes(pkg):
    """8 x 8, A = 64, Q = 1, Philox spectral noise, L = 28 (~100 MB): the echo grid the context re-forms (never stored) against the stored one."""
    sc = make_scene(n_ants=64, n_slots=2, num_slots_param=6, with_noise=False, zero_s_slots=False, seed=31)
    sc.cell.gNBSenAntenna = SimpleNamespace(kind="upa", nV=8, nH=8, dV=0.5, dH=0.5)
    rp, cf = _blocks(pkg, sc)
    est_mod = pkg.sensing.estimation
    c = pkg.Context()
    c.set_upa_doa(True)
    try:
        d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
        kw = dict(nfft=4096, fuse_fft2d=(rp, cf, d_txg), ctx=c, seed=77, noise_domain="spectral")
        arr = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, **kw)
        est_mod.fft2D(rp, cf, arr, d_txg, reuse_range=True, ctx=c)
        stored = est_mod.cleanTargets(c, snapshots=True, residual=True)
        lz = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, lazy=True, **kw)
        est_mod.fft2D(rp, cf, lz, d_txg, reuse_range=True, ctx=c)
        lazy = est_mod.cleanTargets(c, snapshots=True, residual=True)
        assert stored["n_total"] >= 1 and (stored["status"] == 0).all() and "ele" in stored
        _same(lazy, stored)
    finally:
        c.close()


def test_contract(pkg):
    """ISAC_ERR_INVALID_ARG (1) before any fft2D, for max_iter outside 1 .. ISAC_MAX_TARGETS, a negative span, a negative or non-finite tolerance, a mask without an active
    symbol, every NULL required array, a UPA without ele, and after the range stage has rewritten the rows; a refused call leaves the CPI and the next answer as they were."""
    L = pkg._lib
    scene = "upa2x2_24prb"
    sc = K.make(scene)
    s = K.oracle_rows(scene)
    rp, cf = _blocks(pkg, sc)
    est_mod = pkg.sensing.estimation
    c = pkg.Context()
    try:
        dims = (s.g.n_rows, sc.A)
        assert _raw(pkg, c, sc.L, dims=dims)[0] == INVALID_ARG                # before any fft2D
        d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
        echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c)
        with pytest.raises(pkg.IsacError) as e:                             # ISAC_OPT_UPA_DOA off: fft2D refuses its own DoA stage and has still collected the CPI
            est_mod.fft2D(rp, cf, echo, d_txg, ctx=c)
        assert e.value.name == "UNSUPPORTED"
        st, full = _raw(pkg, c, sc.L)
        want = K.oracle_clean(scene)
        assert st == 0 and full.n_iter == want.n_iter and np.array_equal(full.row[:full.n_iter], want.row)
        for kw in (dict(max_iter=0), dict(max_iter=-1), dict(max_iter=L.ISAC_MAX_TARGETS + 1, cap=1), dict(span_rows=-1), dict(merge_tol=-1.0), dict(merge_tol=float("nan")),
                   dict(merge_tol=float("inf")), dict(sym_active=np.zeros(sc.L))):
            assert _raw(pkg, c, sc.L, **kw)[0] == INVALID_ARG, kw
        for k in ("m", "n_iter", "n_kept", "n_left") + INT_KEYS + F64_KEYS:   # ele: a planar array needs it
            assert _raw(pkg, c, sc.L, null=(k,))[0] == INVALID_ARG, k
        st, opt = _raw(pkg, c, sc.L, null=("snapshots", "residual"))         # the two optional arrays
        assert st == 0 and opt.nu.tobytes() == full.nu.tobytes()
        st, big = _raw(pkg, c, sc.L, max_iter=L.ISAC_MAX_TARGETS)            # ISAC_MAX_TARGETS itself is served
        assert st == 0 and big.n_iter == full.n_iter and big.nu[:big.n_iter].tobytes() == full.nu[:full.n_iter].tobytes()
        st, wide = _raw(pkg, c, sc.L, span_rows=2 ** 31 - 1)                 # a span wider than the window: clipped to it
        assert st == 0 and wide.n_iter >= 1
        one = np.zeros(sc.L)
        one[3] = 1
        assert _raw(pkg, c, sc.L, sym_active=one)[0] == 0                    # one active symbol is enough
        with pytest.raises(pkg.IsacError) as e:
            est_mod.cleanTargets(c, mergeTol=-1)
        assert e.value.name == "INVALID_ARG"
        for bad in (dict(symActive=np.ones(sc.L + 1)), dict(residual=True, nSymbols=sc.L + 1), dict(symActive=np.ones(sc.L + 1), nSymbols=sc.L + 1)):
            with pytest.raises(ValueError):                                  # the wrapper knows L from the fft2D call on this context
                est_mod.cleanTargets(c, **bad)
        assert "ele" in est_mod.cleanTargets(c, CustomThresholdFactor=1e300, ThresholdFactor="Custom")   # a planar array: the key is there with no entry at all
        st, again = _raw(pkg, c, sc.L)                                       # none of the refusals disturbed the CPI; the scratch is reused
        assert st == 0 and all(getattr(again, k).tobytes() == getattr(full, k).tobytes() for k in INT_KEYS + F64_KEYS + ("snapshots", "residual"))
        # the range stage alone on OTHER grids rewrites the range rows: no stale answer
        im = import_module
        ep, cfb = im(pkg.__name__ + ".sensing._marshal").est_block(rp), im(pkg.__name__ + ".sensing.estimation.fft2D")._cfar_block(cf)
        other = c.to_device(np.asfortranarray(sc.tx_grid[:, ::-1, :]))
        c.check(c.lib.isac_fft2d_range_stage_dev(c.handle, C.byref(ep), C.byref(cfb), other, d_txg, sc.K, sc.L, sc.A))
        assert _raw(pkg, c, sc.L, dims=dims)[0] == INVALID_ARG
    finally:
        c.close()


@pytest.mark.parametrize("guard,train", [((2, 0), (1, 0)), ((0, 2), (0, 1))])
def test_a_halo_of_zero_is_unsupported(pkg, guard, train):
    """guard + training = 0 in one dimension: fft2D completes, the window carries no neighbours there, the local-maximum test cannot be made."""
    sc = K.make("a4_24prb_generic")
    rp, cf = _blocks(pkg, sc)
    cf.cfarDetector2D.GuardBandSize, cf.cfarDetector2D.TrainingBandSize = tuple(guard), tuple(train)
    c = pkg.Context()
    try:
        d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
        echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c)
        try:
            pkg.sensing.estimation.fft2D(rp, cf, echo, d_txg, ctx=c)
        except pkg.IsacError as e:                                          # a CPI without a detection is still a completed one
            if e.name != "NO_DETECTION":
                raise
        assert _raw(pkg, c, sc.L)[0] == UNSUPPORTED
        with pytest.raises(pkg.IsacError) as e:
            pkg.sensing.estimation.cleanTargets(c)
        assert e.value.name == "UNSUPPORTED" and "isac_fft2d_clean_targets" in str(e.value) and "halo" in str(e.value)
    finally:
        c.close()


def test_the_refinements_lds_refusal_is_the_calls(pkg):
    """nFFT = 16 against L = 112 symbols: the refinement's probe table, (2 M + 2) L phasors with M = ceil(8 L / nFFT) = 56, is 204 KB and does not fit the 160 KB of LDS.
    refineTargets refuses such a CPI; cleanTargets, which runs the same device code on its residual rows, refuses it the same way and before any pass."""
    sc = make_scene(n_ants=4, n_slots=8, nrb=24, num_slots_param=1, seed=24, **T._TWO24)
    rp, cf = _blocks(pkg, sc)
    assert (int(rp.nFFT), sc.L) == (16, 112)
    c = pkg.Context()
    try:
        d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
        echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c)
        try:
            pkg.sensing.estimation.fft2D(rp, cf, echo, d_txg, ctx=c)
        except pkg.IsacError as e:                                          # a CPI without a detection is still a completed one
            if e.name != "NO_DETECTION":
                raise
        row0, col0 = int(cf.CUTIdx[0][0]), int(cf.CUTIdx[1][0])
        with pytest.raises(pkg.IsacError) as e:
            pkg.sensing.estimation.refineTargets(c, dict(row=[row0], col=[col0]))
        assert e.value.name == "UNSUPPORTED"
        st, o = _raw(pkg, c, sc.L)
        assert st == UNSUPPORTED and (o.row == -7).all()
        with pytest.raises(pkg.IsacError) as e:
            pkg.sensing.estimation.cleanTargets(c)
        assert e.value.name == "UNSUPPORTED" and "isac_fft2d_clean_targets" in str(e.value) and "LDS" in str(e.value)
    finally:
        c.close()


def test_a_planar_array_of_more_than_256_elements_is_unsupported(pkg):
    """16 x 17 elements (A = 272) at 24 PRB: with ISAC_OPT_UPA_DOA off fft2D refuses its own DoA stage after it has collected the CPI, so the context holds a completed
    fft2D of a planar array the 2-D scan does not serve.  The call refuses it before any pass and writes nothing -- no output array, no counter."""
    sc = make_scene(n_ants=272, n_slots=2, nrb=24, num_slots_param=6, seed=48, **T._TWO24)
    sc.cell.gNBSenAntenna = SimpleNamespace(kind="upa", nV=16, nH=17, dV=0.5, dH=0.5)
    rp, cf = _blocks(pkg, sc)
    c = pkg.Context()
    try:
        d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
        echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c)
        with pytest.raises(pkg.IsacError) as e:
            pkg.sensing.estimation.fft2D(rp, cf, echo, d_txg, ctx=c)
        assert e.value.name == "UNSUPPORTED"
        assert _dims(c)[2] == 272                                           # the CPI is there
        st, o = _raw(pkg, c, sc.L)
        assert st == UNSUPPORTED and (o.n_iter, o.n_kept, o.n_left) == (-7, -7, -7)
        assert all((getattr(o, k) == -7).all() for k in INT_KEYS) and all(np.isnan(getattr(o, k)).all() for k in F64_KEYS) and not o.snapshots.any() and not o.residual.any()
        with pytest.raises(pkg.IsacError) as e:
            pkg.sensing.estimation.cleanTargets(c)
        assert e.value.name == "UNSUPPORTED" and "256" in str(e.value)
    finally:
        c.close()
