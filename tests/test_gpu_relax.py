"""isac_fft2d_relax_targets on the MI355X: the joint re-fit (RELAX) of Doppler tones on the range rows of the last fft2D (project-defined -- include/isac_relax.h,
DESIGN.md section 5).

Cases and scenes come from tests/_relax_restatement.py; tests/test_relax_cpu.py has shown on the oracle that every bracket decision of every cycle of every case clears
its margin by 1e-6 or more (the measured minimum is 5.2e-3), so nothing here is left out or skipped.  The restatement runs on the DEVICE's own range rows, read through
cleanTargets(..., residual=True) with a threshold no cell exceeds.  Each scene runs fft2D once per module and all its cases behind it."""
from __future__ import annotations

import ctypes as C
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import make_scene

import _relax_restatement as X
import _target_list_restatement as T
import _target_list_upa_restatement as TU

pytestmark = pytest.mark.gpu

NU_TOL = 1e-6          # |nu_dev - nu_ref| L: the NU_TOL of tests/test_gpu_refine.py
FIELD_TOL = 1e-10      # the project's field tolerance, of the field's maximum
INVALID_ARG, UNSUPPORTED = 1, 7
F64_KEYS = ("nu", "vel", "power", "shift", "last_step", "azi", "ele")
NEVER = dict(ThresholdFactor="Custom", CustomThresholdFactor=1e300)       # a threshold no cell exceeds: cleanTargets returns the copy of the range rows untouched
EVERY_CYCLE = ("pair_box2", "off_the_lobe", "edge_rows", "sixty_four")    # cases with failed brackets: the decisions of EVERY cycle are compared (status after c cycles)


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


def _raw(c, L, row, nu_in, dims=None, cycles=X.CYCLES, span_rows=X.SPAN_ROWS, box=X.BOX, sym_active=None, null=(), n=None):
    """The C call itself: (status code, namespace of the raw outputs).  ``null``: the arguments passed as NULL; ``dims``: (nr, A) when the context holds no CPI to ask."""
    nr, A = dims if dims is not None else (_dims(c)[0], _dims(c)[2])
    row, nu_in = np.ascontiguousarray(row, dtype=np.int32), np.ascontiguousarray(nu_in, dtype=np.float64)
    n = row.size if n is None else n
    cap = max(row.size, 1)
    o = SimpleNamespace(status=np.full(cap, -7, dtype=np.int32), **{k: np.full(cap, np.nan) for k in F64_KEYS}, snapshots=np.zeros((A, cap), dtype=np.complex128, order="F"),
                        residual=np.zeros((nr, L, A), dtype=np.complex128, order="F"), row=row, nu_in=nu_in)
    act = None if sym_active is None else np.ascontiguousarray(sym_active, dtype=np.uint8)
    p = lambda k: None if k in null else getattr(o, k).ctypes.data_as(C.c_void_p)    # noqa: E731
    st = c.lib.isac_fft2d_relax_targets(c.handle, p("row"), p("nu_in"), n, cycles, span_rows, box, None if act is None else act.ctypes.data_as(C.c_void_p), p("status"),
                                        *(p(k) for k in F64_KEYS), p("snapshots"), p("residual"))
    return st, o


def _untouched(o):
    return (o.status == -7).all() and all(np.isnan(getattr(o, k)).all() for k in F64_KEYS) and not o.snapshots.any() and not o.residual.any()


def _lists(pkg, c, upa):
    """What the other getters of the CPI return: the list (with snapshots), its refinement, cleanTargets' answer and -- a ULA -- the re-detection."""
    est = pkg.sensing.estimation
    tl = (est.targetListUPA if upa else est.targetList)(c, snapshots=True)
    out = {"tl": tl, "refine": est.refineTargets(c, tl, snapshots=True), "clean": est.cleanTargets(c, maxIter=4, snapshots=True, residual=True)}
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


def _fft2d(pkg, c, sc, rp, cf):
    d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
    echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c)
    try:
        pkg.sensing.estimation.fft2D(rp, cf, echo, d_txg, ctx=c)
    except pkg.IsacError as e:                                              # a CPI without a detection is still a completed one
        if e.name != "NO_DETECTION":
            raise
    return echo, d_txg, d_wave


_runs = {}


def _scene(pkg, ctx, scene):
    """Scene through monoStaticSensing -> isac_fft2d_dev, then: the other getters, the device's range rows, every case of the scene twice (the C call), the per-cycle
    status of the cases of EVERY_CYCLE, the other getters again.  Once per module (host copies only)."""
    if scene not in _runs:
        sc = X.make(scene)
        rp, cf = _blocks(pkg, sc)
        cf = T.with_bands(scene, cf)                                         # the default bands for every scene but X.BANDS_SCENE
        est_mod = pkg.sensing.estimation
        bufs = _fft2d(pkg, ctx, sc, rp, cf)
        before = _lists(pkg, ctx, X.is_upa(scene))
        rows0 = est_mod.cleanTargets(ctx, residual=True, **NEVER)["residual"]
        raw, twice, per_cycle = {}, {}, {}
        for case, (s, _, kw) in X.CASES.items():
            if s != scene:
                continue
            row, nu = X.entries(case)
            for store in (raw, twice):
                st, store[case] = _raw(ctx, sc.L, row, nu, **kw)
                assert st == 0, (case, st)
            if case in EVERY_CYCLE:
                per_cycle[case] = [_raw(ctx, sc.L, row, nu, **{**kw, "cycles": c})[1].status for c in range(1, kw.get("cycles", X.CYCLES) + 1)]
        after = _lists(pkg, ctx, X.is_upa(scene))
        for d in bufs:
            d.free()
        _runs[scene] = SimpleNamespace(sc=sc, rp=rp, cf=cf, rows0=rows0, raw=raw, twice=twice, per_cycle=per_cycle, before=before, after=after)
    return _runs[scene]


_want = {}


def _case(pkg, ctx, case):
    """(the scene's run, the device's raw outputs, the restatement on the device's own rows)."""
    r = _scene(pkg, ctx, X.CASES[case][0])
    if case not in _want:
        _want[case] = X.run(case, r.rows0)
    return r, r.raw[case], _want[case]


@pytest.mark.parametrize("scene", list(X.SCENES))
def test_device_rows_are_the_oracles(pkg, ctx, scene):
    """The rows the restatement runs on: the device's ymid window, within 1e-10 of the maximum of the oracle's (so the conditioning shown on the oracle holds for them);
    a call with n = 0 returns the same bytes."""
    r, s = _scene(pkg, ctx, scene), X.oracle_rows(scene)
    err = np.abs(r.rows0 - s.rows).max() / np.abs(s.rows).max()
    print(f"{scene}: rows [{' x '.join(map(str, r.rows0.shape))}] against the oracle's {err:.3e} of the maximum")
    assert r.rows0.shape == s.rows.shape == (s.g.n_rows, X.n_symbols(scene), r.sc.A) and err <= FIELD_TOL


@pytest.mark.parametrize("case", list(X.CASES))
def test_decisions_equal_the_restatement(pkg, ctx, case):
    """status equals the restatement's on the device's own rows -- for the cases with failed brackets after every number of cycles, which is every bracket decision of the
    call.  A flipped decision elsewhere moves nu by a lobe's fraction: test_values_against_the_restatement holds it to 1e-6."""
    r, raw, want = _case(pkg, ctx, case)
    print(f"{case}: status {raw.status.tolist()}; brackets failed {int((~want.decisions).sum())} of {want.decisions.size}; smallest margin on the device's rows "
          f"{want.margins.min() if want.margins.size else np.inf:.3e}")
    assert np.array_equal(raw.status, want.status)
    if case in EVERY_CYCLE:
        got = np.stack(r.per_cycle[case]) == 0
        assert got.shape == want.decisions.shape and np.array_equal(got, want.decisions)
        assert not want.decisions.all()


@pytest.mark.parametrize("case", list(X.CASES))
def test_values_against_the_restatement(pkg, ctx, case):
    """|nu_dev - nu_ref| L <= 1e-6; residual_rows, snapshots and power within 1e-10 of the field's maximum; vel, shift exactly the header's expressions of nu; last_step within
    the two nu tolerances; azi (ele) = the lists' restatement of the Bartlett scan on the device's own snapshots, exactly."""
    r, raw, want = _case(pkg, ctx, case)
    s = X.oracle_rows(X.CASES[case][0])
    L = s.L
    e_nu = np.abs(raw.nu - want.nu).max() * L
    e_res = np.abs(raw.residual - want.residual).max() / np.abs(r.rows0).max()
    e_snap = np.abs(raw.snapshots - want.snapshots).max() / np.abs(want.snapshots).max()
    e_pow = np.abs(raw.power - want.power).max() / want.power.max()
    print(f"{case}: nu error {e_nu:.3e} / L, residual {e_res:.3e}, snapshots {e_snap:.3e}, power {e_pow:.3e} of the field maxima; last step {raw.last_step.max():.3e}")
    assert e_nu <= NU_TOL
    assert e_res <= FIELD_TOL and e_snap <= FIELD_TOL and e_pow <= FIELD_TOL
    assert np.array_equal(raw.vel, raw.nu * s.g.n_fft * float(r.rp.vRes)) and np.array_equal(raw.shift, np.abs(raw.nu - raw.nu_in) * L)
    assert np.abs(raw.last_step - want.last_step).max() <= 2 * NU_TOL
    if X.is_upa(X.CASES[case][0]):
        _, azi, ele, _, _ = TU.bartlett2d(raw.snapshots, r.sc.nV, r.sc.nH, r.rp)
        assert np.array_equal(raw.azi, azi) and np.array_equal(raw.ele, ele)
    else:
        _, azi, _, _ = T.bartlett(raw.snapshots, r.rp)
        assert np.array_equal(raw.azi, azi) and np.isnan(raw.ele).all()      # a ULA: ele is not written


@pytest.mark.parametrize("scene", list(X.SCENES))
def test_determinism_and_untouched_getters(pkg, ctx, scene):
    """Two calls give the same bytes in every output; targetList, refineTargets, redetect and cleanTargets return after the calls the bytes they returned before them;
    rows outside every span keep the bytes of the range rows."""
    r = _scene(pkg, ctx, scene)
    for case, a in r.raw.items():
        b = r.twice[case]
        assert all(getattr(a, k).tobytes(order="A") == getattr(b, k).tobytes(order="A") for k in ("status",) + F64_KEYS + ("snapshots", "residual")), case
        kw = X.CASES[case][2]
        g = X.oracle_rows(scene).g
        touched = sorted({w for lo, hi in X.spans(a.row - g.first_row, g.n_rows, kw.get("span_rows", X.SPAN_ROWS)) for w in range(lo, hi + 1)})
        rest = np.setdiff1d(np.arange(g.n_rows), touched)
        assert a.residual[rest].tobytes() == r.rows0[rest].tobytes() and np.abs(a.residual[touched] - r.rows0[touched]).max() > 0, case
    _same(r.before, r.after)


def test_python_dict_and_the_chain_from_clean(pkg, ctx):
    """sensing.estimation.relaxTargets returns the C call's answer in a dict getRMSE takes; it takes cleanTargets' dict as it stands; with cycles = 0 its residual is
    cleanTargets' own for the same entries (merge_tol 0: every extracted entry is in the dict) to 1e-10 of the maximum; n = 0 returns the range rows."""
    r = _scene(pkg, ctx, "a4_L28")
    sc = r.sc
    est_mod = pkg.sensing.estimation
    bufs = _fft2d(pkg, ctx, sc, r.rp, r.cf)                                 # (the module's context has moved on to other scenes)
    try:
        row, nu = X.entries("pair")
        raw = r.raw["pair"]
        d = est_mod.relaxTargets(ctx, dict(row=row, nu=nu, col=[33, 34]), snapshots=True, residual=True)
        for k in ("nu", "vel", "power", "shift", "last_step", "azi", "status"):
            assert d[k].tobytes() == getattr(raw, k).tobytes(), k
        assert d["snapshots"].tobytes(order="F") == raw.snapshots.tobytes(order="F") and d["residual"].tobytes(order="F") == raw.residual.tobytes(order="F")
        assert d["row"].tolist() == row.tolist() and d["col"].tolist() == [33, 34] and np.isnan(d["rng"]).all() and "ele" not in d
        cl = est_mod.cleanTargets(ctx, maxIter=4, mergeTol=0, residual=True)
        n = cl["row"].size
        assert n == cl["n_total"] >= 2 and (cl["status"] == 0).all()
        zero = est_mod.relaxTargets(ctx, cl, cycles=0, residual=True)
        err = np.abs(zero["residual"] - cl["residual"]).max() / np.abs(r.rows0).max()
        print(f"cycles = 0 after cleanTargets ({n} entries): residual against cleanTargets' own {err:.3e} of the maximum; bytes equal: {zero['residual'].tobytes() == cl['residual'].tobytes()}")
        assert err <= FIELD_TOL and zero["nu"].tobytes() == cl["nu"].tobytes() and not zero["shift"].any() and not zero["status"].any()
        full = est_mod.relaxTargets(ctx, cl)
        assert full["rng"].tobytes() == cl["rng"].tobytes() and full["col"].tolist() == cl["col"].tolist() and full["row"].tolist() == cl["row"].tolist()
        rm = pkg.sensing.postProcessing.getRMSE(full, r.rp)
        assert rm.velRMSE.size == n and np.isfinite(rm.rngRMSE).all()
        truth = X.true_nu(sc) * float(r.rp.nFFT) * float(r.rp.vRes)
        print(f"truth {truth.round(3).tolist()} m/s: cleanTargets {cl['vel'].round(3).tolist()}, re-fitted {full['vel'].round(3).tolist()}; last step {full['last_step'].tolist()}")
        st, none = _raw(ctx, sc.L, [], [])
        assert st == 0 and none.residual.tobytes(order="F") == r.rows0.tobytes(order="F") and (none.status == -7).all()
        empty = est_mod.relaxTargets(ctx, dict(row=[], nu=[]), residual=True)
        assert empty["row"].size == 0 and empty["residual"].tobytes(order="F") == r.rows0.tobytes(order="F")
        for bad in (dict(symActive=np.ones(sc.L + 1)), dict(residual=True, nSymbols=sc.L + 1)):
            with pytest.raises(ValueError):                                  # the wrapper knows L from the fft2D call on this context
                est_mod.relaxTargets(ctx, cl, **bad)
        with pytest.raises(pkg.IsacError) as e:
            est_mod.relaxTargets(ctx, cl, box=0)
        assert e.value.name == "INVALID_ARG"
    finally:
        for b in bufs:
            b.free()


def test_contract(pkg):
    """ISAC_ERR_INVALID_ARG (1) before any fft2D, for n outside 0 .. ISAC_RELAX_MAX_TONES, cycles outside 0 .. 64, a negative span, a box that is not finite, <= 0 or > 2,
    a nu_in that is not finite, a row outside the CUT zone, a mask without an active symbol, every NULL required array, a UPA without ele, and after the range stage has
    rewritten the rows; a refused call writes nothing and leaves the CPI and the next answer as they were."""
    L = pkg._lib
    scene = "upa2x2_L28"
    sc, s = X.make(scene), X.oracle_rows(scene)
    rp, cf = _blocks(pkg, sc)
    row, nu = X.entries("upa2x2")
    c = pkg.Context()
    try:
        dims = (s.g.n_rows, sc.A)
        assert _raw(c, sc.L, row, nu, dims=dims)[0] == INVALID_ARG            # before any fft2D
        assert _raw(c, sc.L, [], [], dims=dims)[0] == INVALID_ARG             # ... also with n = 0: the context holds nothing
        d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
        echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c)
        with pytest.raises(pkg.IsacError) as e:                             # ISAC_OPT_UPA_DOA off: fft2D refuses its own DoA stage and has still collected the CPI
            pkg.sensing.estimation.fft2D(rp, cf, echo, d_txg, ctx=c)
        assert e.value.name == "UNSUPPORTED"
        st, full = _raw(c, sc.L, row, nu)
        assert st == 0 and (full.status == 0).all() and not np.isnan(full.ele).any()
        r0, r1 = s.g.rect[0], s.g.rect[1]
        bad = [dict(cycles=-1), dict(cycles=65), dict(span_rows=-1), dict(box=0.0), dict(box=-0.5), dict(box=2.5), dict(box=float("nan")), dict(box=float("inf")),
               dict(sym_active=np.zeros(sc.L)), dict(n=-1)]
        for kw in bad:
            st, o = _raw(c, sc.L, row, nu, **kw)
            assert st == INVALID_ARG and _untouched(o), kw
        for v in (float("nan"), float("inf")):
            st, o = _raw(c, sc.L, row, [nu[0], v])
            assert st == INVALID_ARG and _untouched(o), v
        for rr in (r0 - 1, r1 + 1, 0, -3):
            st, o = _raw(c, sc.L, [row[0], rr], nu)
            assert st == INVALID_ARG and _untouched(o), rr                   # outside the CUT zone
        big = np.full(L.ISAC_RELAX_MAX_TONES + 1, row[0], dtype=np.int32)
        st, o = _raw(c, sc.L, big, np.linspace(-0.4, 0.4, big.size))
        assert st == INVALID_ARG and _untouched(o)                           # n > ISAC_RELAX_MAX_TONES
        for k in ("row", "nu_in", "status", "nu", "vel", "power", "shift", "last_step", "azi", "ele"):   # ele: a planar array needs it
            st, o = _raw(c, sc.L, row, nu, null=(k,))
            assert st == INVALID_ARG and _untouched(o), k
        st, opt = _raw(c, sc.L, row, nu, null=("snapshots", "residual"))     # the two optional arrays
        assert st == 0 and opt.nu.tobytes() == full.nu.tobytes()
        for kw in (dict(cycles=0), dict(cycles=64), dict(box=2.0), dict(span_rows=2 ** 31 - 1, cycles=1)):
            assert _raw(c, sc.L, row, nu, **kw)[0] == 0, kw                   # the ends of the ranges are served
        for rr in (r0, r1):
            assert _raw(c, sc.L, [rr], [0.01], cycles=1)[0] == 0, rr         # the first and the last CUT row are inside
        one = np.zeros(sc.L)
        one[3] = 1
        assert _raw(c, sc.L, row, nu, sym_active=one, cycles=1)[0] == 0      # one active symbol is enough
        st, again = _raw(c, sc.L, row, nu)                                   # none of the refusals disturbed the CPI; the scratch is reused
        assert st == 0 and all(getattr(again, k).tobytes(order="A") == getattr(full, k).tobytes(order="A") for k in ("status",) + F64_KEYS + ("snapshots", "residual"))
        # the range stage alone on OTHER grids rewrites the range rows: no stale answer
        im = import_module
        ep, cfb = im(pkg.__name__ + ".sensing._marshal").est_block(rp), im(pkg.__name__ + ".sensing.estimation.fft2D")._cfar_block(cf)
        other = c.to_device(np.asfortranarray(sc.tx_grid[:, ::-1, :]))
        c.check(c.lib.isac_fft2d_range_stage_dev(c.handle, C.byref(ep), C.byref(cfb), other, d_txg, sc.K, sc.L, sc.A))
        st, o = _raw(c, sc.L, row, nu, dims=dims)
        assert st == INVALID_ARG and _untouched(o)
    finally:
        c.close()


def test_the_refinements_lds_refusal_is_the_calls(pkg):
    """nFFT = 16 against L = 112 symbols: the refinement's probe table is 204 KB and does not fit the 160 KB of LDS.  refineTargets refuses such a CPI; the re-fit, whose
    kernels would need 3.7 KB, takes the refinement's rule and refuses it the same way, before any work."""
    sc = make_scene(n_ants=4, n_slots=8, nrb=24, num_slots_param=1, seed=24, **T._TWO24)
    rp, cf = _blocks(pkg, sc)
    assert (int(rp.nFFT), sc.L) == (16, 112)
    c = pkg.Context()
    try:
        _fft2d(pkg, c, sc, rp, cf)
        row0 = int(cf.CUTIdx[0][0])
        st, o = _raw(c, sc.L, [row0], [0.01])
        assert st == UNSUPPORTED and _untouched(o)
        with pytest.raises(pkg.IsacError) as e:
            pkg.sensing.estimation.relaxTargets(c, dict(row=[row0], nu=[0.01]))
        assert e.value.name == "UNSUPPORTED" and "isac_fft2d_relax_targets" in str(e.value) and "LDS" in str(e.value)
        assert _raw(c, sc.L, [], [])[0] == 0                                # n = 0 asks for no kernel
    finally:
        c.close()


def test_a_planar_array_of_more_than_256_elements_is_unsupported(pkg):
    """16 x 17 elements (A = 272) at 24 PRB: with ISAC_OPT_UPA_DOA off fft2D refuses its own DoA stage after it has collected the CPI.  The call refuses the array before
    any work and writes nothing."""
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
        st, o = _raw(c, sc.L, [int(cf.CUTIdx[0][0])], [0.01])
        assert st == UNSUPPORTED and _untouched(o)
        with pytest.raises(pkg.IsacError) as e:
            pkg.sensing.estimation.relaxTargets(c, dict(row=[int(cf.CUTIdx[0][0])], nu=[0.01]))
        assert e.value.name == "UNSUPPORTED" and "256" in str(e.value)
    finally:
        c.close()
