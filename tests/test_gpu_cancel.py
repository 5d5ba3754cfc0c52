"""Reference-signal cancellation on the received waveform, on the device (project-defined: include/isac_cancel_paths.h; csrc/cancel_paths.hip).

RTOL = 1e-10, the project's bound for complex fp64 fields: ||Y' - Y'_ref|| against ||Y|| (the rounding of a difference scales with what is subtracted), coefficients and
powers relative to themselves.  The device solves the normal equations by Cholesky, the restatement (tests/_cancel_restatement.py) uses numpy.linalg.lstsq: at cond(G) <= 1e3,
asserted first, the two differ by about 1e-13.  Every comparison prints what it measured.
  1. edge shapes against the restatement: T 1000 / 4099 (no multiples of 256) / 30 720, 1 / 3 / 4 elements, 1 / 9 / 16 / 17 / 32 references on two sources of 2 and 3 elements
  2. the same bits from two calls and from in place / out of place; loading = 0.1 against the loaded normal equations
  3. the `interference` scene end to end: multiStaticChannel -> cancelPaths(referencePaths(paths)) -> ofdmDemodulate -> fft2D with the cell's own grid, against the oracle
  4. refusals: status, *dependent, and a poison-filled output left untouched"""
from __future__ import annotations

import ctypes as C
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest

import _cancel_restatement as X
import _multistatic_restatement as M
from conftest import load_pkg

pytestmark = pytest.mark.gpu
RTOL = 1e-10
MARGIN = 1e-6


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def _bits(x):
    return np.ascontiguousarray(np.asarray(x).ravel(order="K")).view(np.uint64)


def _fro(got, want, scale):
    return float(np.linalg.norm(np.asarray(got) - np.asarray(want)) / np.linalg.norm(scale))


def _against(name, got, info, want, Y):
    e_out, e_coef = _fro(got, want.out, Y), _fro(info.coef, want.coef, want.coef)
    e_pow = float(max(np.abs(info.power_in / want.power_in - 1.0).max(), np.abs(info.power_out / want.power_out - 1.0).max()))
    print(f"{name}: |Y' - ref| / |Y| = {e_out:.3e}, coef {e_coef:.3e}, power {e_pow:.3e}; removed {np.round(info.removed_dB, 2).tolist()} dB")
    assert got.shape == want.out.shape and info.coef.shape == want.coef.shape
    assert e_out <= RTOL and e_coef <= RTOL and e_pow <= RTOL
    assert np.array_equal(info.removed_dB, 10.0 * np.log10(info.power_in / info.power_out))


# ---------------------------------------------------------------- 1. edge shapes against the restatement
@pytest.mark.parametrize("name", list(X.EDGE_CASES))
def test_edge_shapes_against_the_restatement(pkg, name):
    e = X.edge_case(name)
    print(f"{name}: cond(G) = {e.cond:.3g}")
    assert e.cond <= 1e3
    ctx = pkg.default_context()
    waves = [ctx.to_device(w) for w in e.waves]
    got, info = pkg.sensing.cancelPaths(ctx.to_device(e.Y), waves, e.rp, e.refs, ctx=ctx, return_info=True)
    _against(name, got.numpy(), info, e.want, e.Y)
    host = pkg.sensing.cancelPaths(e.Y, e.waves, e.rp, e.refs, ctx=ctx)     # NumPy in, NumPy out: the same call
    assert isinstance(host, np.ndarray) and np.array_equal(_bits(host), _bits(got.numpy()))


# ---------------------------------------------------------------- 2. bit-level checks
@pytest.mark.parametrize("name", ["t4099_a3_m17", "t30720_a4_m32"])
def test_same_bits_every_time_and_in_place(pkg, name):
    e = X.edge_case(name)
    ctx = pkg.default_context()
    waves = [ctx.to_device(w) for w in e.waves]
    d_y = ctx.to_device(e.Y)
    first, i1 = pkg.sensing.cancelPaths(d_y, waves, e.rp, e.refs, ctx=ctx, return_info=True)
    again, i2 = pkg.sensing.cancelPaths(d_y, waves, e.rp, e.refs, ctx=ctx, return_info=True)
    assert np.array_equal(_bits(d_y.numpy()), _bits(e.Y))                   # out of place: the input is not written
    in_place, i3 = pkg.sensing.cancelPaths(d_y, waves, e.rp, e.refs, out=d_y, ctx=ctx, return_info=True)
    assert in_place is d_y
    a = first.numpy()
    for other, info in ((again.numpy(), i2), (d_y.numpy(), i3)):
        assert np.array_equal(_bits(a), _bits(other))
        assert np.array_equal(_bits(i1.coef), _bits(info.coef)) and np.array_equal(_bits(i1.power_in), _bits(info.power_in)) and np.array_equal(_bits(i1.power_out), _bits(info.power_out))


def test_loading_against_the_loaded_normal_equations(pkg):
    e = X.edge_case("t4099_a4_m16")
    ctx = pkg.default_context()
    got, info = pkg.sensing.cancelPaths(ctx.to_device(e.Y), [ctx.to_device(w) for w in e.waves], e.rp, e.refs, loading=0.1, ctx=ctx, return_info=True)
    _against("loading 0.1", got.numpy(), info, e.want_loaded, e.Y)
    shrink = float(np.linalg.norm(info.coef) / np.linalg.norm(e.want.coef))
    print(f"|C(loading 0.1)| / |C(0)| = {shrink:.4f}")
    assert 0.85 < shrink < 0.95                                              # G is close to a multiple of I here: C shrinks by about 1 / 1.1


# ---------------------------------------------------------------- 3. the interference scene, end to end
def test_interference_scene_end_to_end(pkg):
    s, b = X.interference(), M.base()
    sc = b.sc
    assert all(m > MARGIN for m in s.margin), f"a CUT cell lies within {min(s.margin):.2e} of its threshold"
    ctx = pkg.Context()
    try:
        rp = pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)
        paths = pkg.sensing.channelModels.multiStaticPaths(sc.cell, [sc.cell, b.nb.cell], b.targets, carrierInfo=sc.carrier, waveInfo=sc.wave)
        waves = [ctx.to_device(sc.tx_wave), ctx.to_device(b.nb.tx_wave)]
        rx = pkg.sensing.channelModels.multiStaticChannel(waves, rp, paths, noise=ctx.to_device(sc.noise), ctx=ctx)
        refs = pkg.sensing.channelModels.referencePaths(paths)
        assert refs.shift.tolist() == [X.DIRECT_SAMPLES] and refs.source.tolist() == [1]
        clean, info = pkg.sensing.cancelPaths(rx, waves, rp, refs, ctx=ctx, return_info=True)
        err = _fro(clean.numpy(), s.res.out, s.Y)
        print(f"cancelled waveform against the restatement {err:.3e} of |Y|; removed {info.removed_dB.tolist()} dB")
        assert err <= RTOL
        assert (info.removed_dB > 40.0).all()
        grid = pkg.sensing.ofdmDemodulate(clean, sc.tx_grid.shape, sc.carrier, nfft=sc.wave.Nfft, ctx=ctx)
        assert tuple(grid.shape) == s.echo.shape
        cf = pkg.sensing.detection.cfar2D(rp)
        est, dbg = pkg.sensing.estimation.fft2D(rp, cf, grid, ctx.to_device(sc.tx_grid), return_debug=True, ctx=ctx)
        print(f"detections per antenna {[d.shape[1] for d in dbg.detections]}; rngEst {est.rngEst.tolist()}; aziEst {np.asarray(est.aziEst).tolist()}")
        assert len(dbg.detections) == len(s.dets)
        for a, (d, o) in enumerate(zip(dbg.detections, s.dets)):
            assert np.array_equal(d, o), f"antenna {a}"
        assert np.array_equal(est.rngEst, s.est.rngEst) and np.array_equal(est.velEst, s.est.velEst) and np.array_equal(est.aziEst, s.est.aziEst)
        assert est.rngEst[0] == 33 * sc.rp.rRes
        with pytest.raises(pkg.IsacError) as blind:                          # ... and without the cancellation the cell is blind
            pkg.sensing.estimation.fft2D(rp, cf, pkg.sensing.ofdmDemodulate(rx, sc.tx_grid.shape, sc.carrier, nfft=sc.wave.Nfft, ctx=ctx), ctx.to_device(sc.tx_grid), ctx=ctx)
        assert blind.value.name == "NO_DETECTION"
    finally:
        ctx.close()


# ---------------------------------------------------------------- 4. refusals
T_REF, A_REF = 1000, 3
REFUSALS = {                                                                # name -> (status name, *dependent afterwards (-5: not written), what to break)
    "same_reference_twice": ("INVALID_ARG", 1, dict(twice=True)),
    "shift_at_T": ("INVALID_ARG", 2, dict(shift={2: T_REF})),
    "shift_beyond_T": ("INVALID_ARG", 0, dict(shift={0: T_REF + 77})),
    "no_reference": ("INVALID_ARG", -5, dict(M=0)),
    "too_many_references": ("CAPACITY", -5, dict(M=33)),
    "named_source_without_a_waveform": ("INVALID_ARG", -5, dict(null_wave=1)),
    "source_index_too_large": ("INVALID_ARG", -5, dict(source={1: 2})),
    "negative_shift": ("INVALID_ARG", -5, dict(shift={1: -1})),
    "negative_loading": ("INVALID_ARG", -5, dict(loading=-0.5)),
    "partial_overlap": ("INVALID_ARG", -5, dict(overlap=8)),
    "too_many_receive_elements": ("CAPACITY", -5, dict(A=257)),
}


def _refusal_call(pkg, ctx, brk, in_place=False):
    """The flat call on three valid references (sources of 2 and 3 elements) with one thing broken -> (status, *dependent, the output afterwards, what it held before)."""
    L = pkg._lib
    M_, A = brk.get("M", 3), brk.get("A", A_REF)
    rng = np.random.default_rng(11)
    cn = lambda shape: np.asfortranarray(rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    waves = [ctx.to_device(cn((T_REF, a))) for a in X.A_SRC]
    n_ants_src = np.asarray(X.A_SRC, dtype=np.int32)
    source = (np.arange(max(M_, 1)) % 2).astype(np.int32)
    shift = (5 * np.arange(max(M_, 1))).astype(np.int64)
    doppler = np.zeros(max(M_, 1))
    for k, v in brk.get("shift", {}).items():
        shift[k] = v
    for k, v in brk.get("source", {}).items():
        source[k] = v
    if brk.get("twice"):
        source[1], shift[1] = source[0], shift[0]
    steer = np.ones(int(sum(X.A_SRC[s % 2] for s in source)), dtype=np.complex128)
    ptrs = (C.c_void_p * 2)(*[None if i == brk.get("null_wave", -1) else w.ptr for i, w in enumerate(waves)])
    poison = np.float64(-7.25e300)
    n = T_REF * A
    pool = ctx.to_device(np.concatenate([cn((n,)), np.full(n + 64, poison + 1j * poison)]))   # [Y | poison]: one allocation, so that a partly overlapping d_out stays inside it
    off = brk.get("overlap", n)
    d_rx = L.DeviceArray(ctx, pool.ptr, (T_REF, A), np.complex128, owner=False)
    d_out = d_rx if in_place else L.DeviceArray(ctx, pool.ptr + 16 * off, (T_REF, A), np.complex128, owner=False)
    before = d_out.numpy()
    coef, power, dep = np.full((max(M_, 1), A), 9.0 + 0j, order="F"), np.full((2, A), 9.0), C.c_int32(-5)
    p_ = lambda a: a.ctypes.data_as(C.c_void_p)
    st = ctx.lib.isac_cancel_paths_dev(ctx.handle, ptrs, p_(n_ants_src), 2, T_REF, X.FC, X.FS, A, M_, p_(source), p_(shift), p_(doppler), p_(steer), brk.get("loading", 0.0),
                                       d_rx, d_out, p_(coef), p_(power), C.byref(dep))
    ctx.sync()
    msg = (ctx.lib.isac_last_error(ctx.handle) or b"").decode()
    return SimpleNamespace(st=st, msg=msg, dep=dep.value, before=before, after=d_out.numpy(), coef=coef, power=power, keep=(pool, waves))


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refused_calls_write_nothing(pkg, name):
    status, dep, brk = REFUSALS[name]
    code = {v: k for k, v in pkg._lib.STATUS_NAMES.items()}[status]
    ctx = pkg.Context()
    try:
        for in_place in ((False, True) if "overlap" not in brk else (False,)):
            r = _refusal_call(pkg, ctx, brk, in_place)
            print(f"{name}, {'in place' if in_place else 'out of place'}: status {r.st} ({r.msg}); *dependent {r.dep}")
            assert r.st == code and r.dep == dep, (r.st, r.dep, r.msg)
            assert np.array_equal(_bits(r.after), _bits(r.before)), "a refused call wrote to its output"
            assert (r.coef == 9.0).all() and (r.power == 9.0).all()
    finally:
        ctx.close()


def test_a_valid_call_of_the_refusal_shape_is_accepted(pkg):
    """The arrays the refusals start from, unbroken: ISAC_OK, *dependent = -1, an output that changed -- so each refusal above is caused by what was broken."""
    ctx = pkg.Context()
    try:
        r = _refusal_call(pkg, ctx, {})
        assert r.st == 0 and r.dep == -1, r.msg
        assert not (r.after.real == -7.25e300).any() and (r.coef != 9.0).all() and (r.power[1] < r.power[0]).all()
    finally:
        ctx.close()
