"""Sub-sample range on the MI355X (project-defined -- include/isac_subsample.h): isac_range_refine_dev (csrc/range_refine.hip) and
isac_multi_static_sensing_frac_dev (the ramp of csrc/multistatic.hip behind echo.hip's tails).

Scenes and the restated results come from tests/_subsample_restatement.py; tests/test_subsample_cpu.py has shown without a GPU that every entry's maximiser is conditioned
for the 1e-6 bound (|P'| at rho_ref +- 1e-6 is 1.7e4 rounding bounds or more), that no comparison of the peak rule is closer than 5.9e-4, and that the ramp equals the
physically delayed signal on the "still" scene.
  1. device against the restatement: rho to 1e-6 bin (the project's NU_TOL convention), power to 1e-10 relative, x to 1e-10 of max|x|, rng == rho rRes
  2. probe_only at the cells of refineTargets: x times the range-axis weight of the row is that call's snapshot
  3. an entry alone = the entry among 33; two runs; the context's list and every getter's answer before and after; a pending submit collects the isac_est_result of an
     undisturbed run, byte for byte, after a full and a probe_only call in between
  4. refusals, outputs untouched
  5. the fractional echo: frac NULL / zero = isac_multi_static_sensing_dev's bytes in five noise modes; against (a) with noise and (b) without; the time-domain modes refuse
  6. end to end: multiStaticPaths(subSample=True) -> multiStaticSensing -> fft2D -> targetList -> refineTargets -> refineRange -> getRMSE"""
from __future__ import annotations

import ctypes as C
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest
from scipy import fft as sfft

import _subsample_restatement as S
from oracle.matlab_compat import kaiser

pytestmark = pytest.mark.gpu

RHO_TOL = 1e-6
FIELD_TOL = 1e-10
E2E_BOUND = 0.1                                                             # bins: twice the bound tests/test_subsample_cpu.py holds the restated chain to
POISON = -7.25e300


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context()
    yield c
    c.close()


def _b(x):
    return np.asfortranarray(x).tobytes(order="F")


def _rp(s):
    return SimpleNamespace(nIFFT=s.n_ifft, nFFT=s.n_fft, rRes=s.r_res, vRes=1.0, azimuthScanScale=360, azimuthScanGranularity=1, elevationScanScale=180,
                           elevationScanGranularity=1)


def _refine(pkg):
    return import_module(pkg.__name__ + ".sensing.estimation.refineRange").range_refine


_dev = {}


def _scene_on_device(pkg, ctx, name):
    """The scene's grids on the device and the call on all its entries, once per module."""
    if name not in _dev:
        s = S.tone_scene(name)
        d_rx, d_tx = ctx.to_device(s.rx), ctx.to_device(s.tx)
        _dev[name] = SimpleNamespace(s=s, d_rx=d_rx, d_tx=d_tx, out=_refine(pkg)(ctx, d_rx, d_tx, _rp(s), s.row, s.nu))
    return _dev[name]


# ---------------------------------------------------------------- 1
@pytest.mark.parametrize("name", list(S.SHAPES))
def test_device_against_the_restatement(pkg, ctx, name):
    d = _scene_on_device(pkg, ctx, name)
    s, (status, rho, rng, power, x) = d.s, d.out
    e_rho = float(np.abs(rho - s.ref.rho).max())
    e_p = float(np.abs(power / s.ref.power - 1).max())
    e_x = float((np.abs(x - s.ref.x).max(axis=0) / np.abs(s.ref.x).max(axis=0)).max())
    print(f"{name}: status {status.tolist()}; rho error {e_rho:.3e} bin, power error {e_p:.3e} relative, x error {e_x:.3e} of max|x|; rho {rho.round(4).tolist()}")
    assert (s.K, s.n_ifft, s.L, s.A, s.n) == S.SHAPES[name] and x.shape == (s.A, s.n)
    assert np.array_equal(status, s.ref.status)
    assert e_rho <= RHO_TOL
    assert e_p <= FIELD_TOL
    assert e_x <= FIELD_TOL
    assert np.array_equal(rng, rho * s.r_res)
    assert np.array_equal(rho[status == 1], (s.row[status == 1] - 1).astype(np.float64))


# ---------------------------------------------------------------- 2 and 6 share one chain
_chain = {}


def _e2e(pkg):
    """The end-to-end scene through the package, on a context of its own, once per module."""
    if not _chain:
        sc = S.e2e_scene()
        est = pkg.sensing.estimation
        c = pkg.Context()
        try:
            rp = pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)
            cf = pkg.sensing.detection.cfar2D(rp)
            targets = [SimpleNamespace(position=np.asarray(p, dtype=np.float64), velocity=np.zeros(3), rcs=1.0) for p in sc.cell.targetPosition]
            for t, v in zip(targets, S.E2E_VELOCITY):                       # radial speed v towards the gNB (radarParams' velocity is the speed towards the node)
                d = t.position - sc.cell.gNBPosition
                t.velocity = -v * d / np.sqrt(d @ d)
            kw = dict(carrierInfo=sc.carrier, waveInfo=sc.wave)
            paths = pkg.sensing.channelModels.multiStaticPaths(sc.cell, [sc.cell], targets, subSample=True, **kw)
            ceil = pkg.sensing.channelModels.multiStaticPaths(sc.cell, [sc.cell], targets, **kw)
            d_wave, d_txg = c.to_device(sc.tx_wave), c.to_device(sc.tx_grid)
            echo = pkg.sensing.multiStaticSensing([d_wave], sc.tx_grid.shape, sc.carrier, rp, paths, seed=S.E2E_SEED, noise_domain="spectral", nfft=sc.wave.Nfft, ctx=c)
            pkg.sensing.estimation.fft2D(rp, cf, echo, d_txg, ctx=c)
            tl = est.targetList(c, snapshots=True)
            fine = est.refineTargets(c, tl, snapshots=True)
            dbg = import_module(pkg.__name__ + ".sensing.estimation.fft2D").fft2D_debug(c, sc.A)
            rr = est.refineRange(c, echo, d_txg, rp, fine)
            probe = _refine(pkg)(c, echo, d_txg, rp, fine["row"], fine["nu"], probeOnly=True)
            tl_after = est.targetList(c, snapshots=True)
            dbg_after = import_module(pkg.__name__ + ".sensing.estimation.fft2D").fft2D_debug(c, sc.A)
            rmse = pkg.sensing.postProcessing.getRMSE(rr, rp)
            rmse_grid = pkg.sensing.postProcessing.getRMSE(fine, rp)
            _chain["v"] = SimpleNamespace(sc=sc, rp=rp, cf=cf, paths=paths, ceil=ceil, tl=tl, tl_after=tl_after, dbg=dbg, dbg_after=dbg_after, fine=fine, rr=rr, probe=probe, rmse=rmse,
                                          rmse_grid=rmse_grid)
        finally:
            c.close()
    return _chain["v"]


def test_probe_only_is_the_snapshot_of_refine_targets(pkg):
    v = _e2e(pkg)
    status, rho, rng, power, x = v.probe
    w_eff = sfft.fftshift(kaiser(int(v.rp.nIFFT), 3.0))
    want = v.fine["snapshots"]
    got = x * w_eff[v.fine["row"] - 1][None, :]
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"probe_only at rows {v.fine['row'].tolist()}, nu {v.fine['nu'].tolist()}: x w_eff against refineTargets' snapshots {err:.3e} of max|x|")
    assert want.shape[1] >= 2 and (status == 2).all() and np.array_equal(rho, (v.fine["row"] - 1).astype(np.float64)) and np.array_equal(rng, rho * float(v.rp.rRes))
    assert err <= FIELD_TOL
    assert np.abs(power / ((np.abs(want) ** 2).sum(axis=0) / w_eff[v.fine["row"] - 1] ** 2) - 1).max() <= FIELD_TOL


# ---------------------------------------------------------------- 3
def test_an_entry_does_not_depend_on_the_others(pkg, ctx):
    d = _scene_on_device(pkg, ctx, "k288_l28_a8")
    s = d.s
    again = _refine(pkg)(ctx, d.d_rx, d.d_tx, _rp(s), s.row, s.nu)
    for a, b in zip(d.out, again):
        assert _b(a) == _b(b)                     # two runs
    for i in range(s.n):                                                    # alone: slot 0 of a chunk of its own; among 33: slot i % 16 of chunk i / 16
        one = _refine(pkg)(ctx, d.d_rx, d.d_tx, _rp(s), s.row[i:i + 1], s.nu[i:i + 1])
        for a, b in zip(one, d.out):
            assert _b(a) == _b(b[..., i:i + 1]), i
    rev = _refine(pkg)(ctx, d.d_rx, d.d_tx, _rp(s), s.row[::-1].copy(), s.nu[::-1].copy())
    for a, b in zip(rev, d.out):
        assert _b(a) == _b(b[..., ::-1])           # any position


def test_the_context_keeps_its_lists(pkg):
    v = _e2e(pkg)
    assert sorted(v.tl) == sorted(v.tl_after) and v.tl["row"].size >= 2
    for k in v.tl:
        assert np.asarray(v.tl[k]).tobytes() == np.asarray(v.tl_after[k]).tobytes(), k
    assert len(v.dbg.detections) == len(v.dbg_after.detections) == v.sc.A
    for a, b in zip(v.dbg.detections + v.dbg.det_pow, v.dbg_after.detections + v.dbg_after.det_pow):
        assert a.tobytes() == b.tobytes()
    for k in ("power_window", "Ra", "spectrum_db"):                         # every other getter's answer
        assert getattr(v.dbg, k).tobytes() == getattr(v.dbg_after, k).tobytes(), k
    assert (v.dbg.first_row, v.dbg.first_col) == (v.dbg_after.first_row, v.dbg_after.first_col)


def test_a_pending_submit_and_its_isac_est_result_survive_the_call(pkg):
    """A submitted, uncollected CPI (pending state, result on its way into the context's pinned buffer) while the same context refines ranges, in full and with probe_only:
    the collect then returns the very isac_est_result of an undisturbed submit + collect, byte for byte, and the refined ranges are those of the chain."""
    v = _e2e(pkg)
    sc = v.sc
    F = import_module(pkg.__name__ + ".sensing.estimation.fft2D")
    c = pkg.Context()
    try:
        d_wave, d_txg = c.to_device(sc.tx_wave), c.to_device(sc.tx_grid)
        echo = pkg.sensing.multiStaticSensing([d_wave], sc.tx_grid.shape, sc.carrier, v.rp, v.paths, seed=S.E2E_SEED, noise_domain="spectral", nfft=sc.wave.Nfft, ctx=c)
        ref = pkg._lib.EstResult()
        F.fft2D_submit(v.rp, v.cf, echo, d_txg, ctx=c)
        c.check(c.lib.isac_fft2d_collect(c.handle, C.byref(ref)))
        assert ref.n_rng >= 2
        for probe_only, want in ((False, (v.rr["range_status"], v.rr["rho"], v.rr["rng"], v.rr["range_power"], v.rr["range_snapshots"])), (True, v.probe)):
            F.fft2D_submit(v.rp, v.cf, echo, d_txg, ctx=c)
            got = _refine(pkg)(c, echo, d_txg, v.rp, v.fine["row"], v.fine["nu"], probeOnly=probe_only)
            res = pkg._lib.EstResult()
            c.check(c.lib.isac_fft2d_collect(c.handle, C.byref(res)))
            assert bytes(res) == bytes(ref), probe_only                     # the whole isac_est_result
            for a, b in zip(got, want):
                assert _b(a) == _b(b), probe_only
        tl = pkg.sensing.estimation.targetList(c, snapshots=True)           # and the collected CPI gives the chain's list
        for k in v.tl:
            assert np.asarray(tl[k]).tobytes() == np.asarray(v.tl[k]).tobytes(), k
    finally:
        c.close()


# ---------------------------------------------------------------- 4
REFUSALS = {                                                                # name -> (status name, what to break)
    "null_rx_grid": ("INVALID_ARG", dict(rx=None)),
    "null_tx_grid": ("INVALID_ARG", dict(tx=None)),
    "null_ep": ("INVALID_ARG", dict(ep=None)),
    **{"null_" + k: ("INVALID_ARG", {k: None}) for k in ("row", "nu", "status", "rho", "rng", "power")},
    "negative_n": ("INVALID_ARG", dict(n=-1)),
    "too_many_entries": ("INVALID_ARG", dict(n=1025)),
    "zero_K": ("INVALID_ARG", dict(K=0)),
    "zero_L": ("INVALID_ARG", dict(L=0)),
    "zero_A": ("INVALID_ARG", dict(A=0)),
    "K_above_n_ifft": ("INVALID_ARG", dict(n_ifft=256)),
    "row_zero": ("INVALID_ARG", dict(row1=0)),
    "row_above_n_ifft": ("INVALID_ARG", dict(row1=513)),
    "nu_nan": ("INVALID_ARG", dict(nu1=np.nan)),
    "nu_inf": ("INVALID_ARG", dict(nu1=np.inf)),
    "zero_n_fft": ("INVALID_ARG", dict(n_fft=0)),
    "too_many_antennas": ("CAPACITY", dict(A=257)),
    "too_many_subcarriers": ("UNSUPPORTED", dict(K=8193, n_ifft=16384)),    # the phasors of one evaluation stay in LDS (the header's limit)
}


def _raw_call(pkg, ctx, d, brk):
    """isac_range_refine_dev on the first scene's grids with two valid entries and poison-filled outputs; the caller breaks one thing.  Returns (status, outputs)."""
    L = pkg._lib
    s = d.s
    n = 2
    row, nu = np.array([41, 42], dtype=np.int32), np.array([0.11, 0.12])
    if "row1" in brk:
        row[1] = brk["row1"]
    if "nu1" in brk:
        nu[1] = brk["nu1"]
    ep = L.EstParams(brk.get("n_ifft", s.n_ifft), brk.get("n_fft", s.n_fft), s.r_res, 1.0, 0, 0, 0, 360.0, 1.0, 180.0, 1.0)
    o = SimpleNamespace(status=np.full(n, -7, dtype=np.int32), rho=np.full(n, POISON), rng=np.full(n, POISON), power=np.full(n, POISON),
                        snap=np.full((s.A, n), POISON + 1j * POISON, dtype=np.complex128, order="F"))
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)      # noqa: E731
    arg = dict(rx=d.d_rx, tx=d.d_tx, ep=C.byref(ep), row=row, nu=nu, status=o.status, rho=o.rho, rng=o.rng, power=o.power)
    arg.update({k: v for k, v in brk.items() if k in arg})
    ptr = lambda k: arg[k] if k in ("rx", "tx", "ep") else p(arg[k])       # noqa: E731
    st = ctx.lib.isac_range_refine_dev(ctx.handle, ptr("ep"), ptr("rx"), ptr("tx"), brk.get("K", s.K), brk.get("L", s.L), brk.get("A", s.A), ptr("row"), ptr("nu"),
                                       brk.get("n", n), 0, ptr("status"), ptr("rho"), ptr("rng"), ptr("power"), p(o.snap))
    ctx.sync()
    return st, o


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refused_range_calls_write_nothing(pkg, ctx, name):
    status, brk = REFUSALS[name]
    code = {v: k for k, v in pkg._lib.STATUS_NAMES.items()}[status]
    st, o = _raw_call(pkg, ctx, _scene_on_device(pkg, ctx, "k288_a2"), brk)
    msg = (ctx.lib.isac_last_error(ctx.handle) or b"").decode()
    print(f"{name}: status {st} ({msg})")
    assert st == code, msg
    assert (o.status == -7).all() and all((v == POISON).all() for v in (o.rho, o.rng, o.power, o.snap.real, o.snap.imag))


def test_a_valid_call_of_the_refusal_shape_is_accepted(pkg, ctx):
    """The arguments the refusals start from, unbroken, and n = 0 with NULL arrays: ISAC_OK."""
    d = _scene_on_device(pkg, ctx, "k288_a2")
    st, o = _raw_call(pkg, ctx, d, {})
    assert st == 0 and (o.status >= 0).all() and not (o.rho == POISON).any() and not (o.snap.real == POISON).any() and np.array_equal(o.rng, o.rho * d.s.r_res)
    st, o = _raw_call(pkg, ctx, d, dict(n=0, row=None, nu=None, status=None, rho=None, rng=None, power=None))
    assert st == 0


# ---------------------------------------------------------------- 5
def _cnormal(rng, shape):
    return np.asfortranarray(rng.standard_normal(shape) + 1j * rng.standard_normal(shape))


def _frac_call(pkg, ctx, s, frac, mode, d_noise, seed, d_waves, out):
    """isac_multi_static_sensing_frac_dev itself (frac: an array or None); returns the status."""
    b = import_module(pkg.__name__ + ".sensing.channelModels.multiStaticChannel").PathBlock(ctx, d_waves, s.rp, SimpleNamespace(**{k: v for k, v in vars(s.paths).items() if k != "frac"}))
    car = pkg._lib.Carrier(s.K, s.nfft, s.scs, 0)
    lo = C.c_int32(-5)
    f = None if frac is None else np.ascontiguousarray(frac, dtype=np.float64)
    st = ctx.lib.isac_multi_static_sensing_frac_dev(*b.args[:12], None if f is None else f.ctypes.data_as(C.c_void_p), *b.args[12:], mode, d_noise, seed, out.shape[1], C.byref(car), out,
                                                    C.byref(lo))
    ctx.sync()
    return st, lo.value


def test_zero_fractions_give_the_bytes_of_the_plain_call(pkg, ctx):
    s = S.frac_scene("moving")
    L = pkg._lib
    d_waves = [ctx.to_device(w) for w in s.waves]
    dims = (s.K, s.L + 1, s.A)                                              # one padded column
    rng = np.random.default_rng(8)
    d_nt, d_ns = ctx.to_device(_cnormal(rng, (s.T, s.A))), ctx.to_device(_cnormal(rng, dims))
    plain = SimpleNamespace(**{k: v for k, v in vars(s.paths).items() if k != "frac"})
    modes = {L.NOISE_NONE: (None, 0, {}), L.NOISE_INJECTED: (d_nt, 0, dict(noise=d_nt)), L.NOISE_PHILOX: (None, 77, dict(seed=77)),
             L.NOISE_PHILOX_SPECTRAL: (None, 99, dict(seed=99, noise_domain="spectral")), L.NOISE_INJECTED_SPECTRAL: (d_ns, 0, dict(spectral_noise=d_ns))}
    seen = set()
    for mode, (d_noise, seed, kw) in modes.items():
        want = pkg.sensing.multiStaticSensing(d_waves, dims, s.carrier, s.rp, plain, nfft=s.nfft, ctx=ctx, **kw).numpy()
        seen.add(want.tobytes())
        for frac in (None, np.zeros(3)):
            out = ctx.to_device(np.full(dims, POISON + 1j * POISON, dtype=np.complex128, order="F"))
            st, lo = _frac_call(pkg, ctx, s, frac, mode, d_noise, seed, d_waves, out)
            assert st == 0 and lo == s.L + 1
            assert _b(out.numpy()) == _b(want), (mode, frac)
        zero = SimpleNamespace(**vars(plain), frac=np.zeros(3))             # ... and through the Python mirror: a record with frac takes the new entry point
        got = pkg.sensing.multiStaticSensing(d_waves, dims, s.carrier, s.rp, zero, nfft=s.nfft, ctx=ctx, **kw).numpy()
        assert _b(got) == _b(want), mode
    assert len(seen) == 5


@pytest.mark.parametrize("name", list(S.FRAC_SCENES))
def test_fractional_echo_against_the_restatement(pkg, ctx, name):
    """(a) with injected spectral noise on both scenes; (b), the physical reference, without noise on the scene that is inside its validity limit."""
    s = S.frac_scene(name)
    d_waves = [ctx.to_device(w) for w in s.waves]
    dims = (s.K, s.L, s.A)
    W = _cnormal(np.random.default_rng(9), dims)
    sens = lambda w: pkg.sensing.multiStaticSensing(d_waves, dims, s.carrier, s.rp, s.paths, nfft=s.nfft, ctx=ctx, spectral_noise=w).numpy()   # noqa: E731
    want = s.ramp + np.sqrt(s.rp.N0 / 2.0) * np.sqrt(s.nfft) * W
    e_a = float(np.abs(sens(W) - want).max() / np.abs(want).max())
    quiet = sens(np.zeros(dims))
    e_q = float(np.abs(quiet - s.ramp).max() / np.abs(s.ramp).max())
    print(f"{name}: against (a) with noise {e_a:.3e}, without {e_q:.3e} of max|grid|")
    assert float(np.abs(want - s.ramp).max()) > 0.5 * float(np.abs(s.ramp).max())           # the noise is there
    assert e_a <= FIELD_TOL and e_q <= FIELD_TOL
    if name == "still":
        phys = S.frac_physical(name)
        e_b = float(np.abs(quiet - phys).max() / np.abs(phys).max())
        print(f"{name}: against (b), the physical reference, {e_b:.3e} of max|grid|")
        assert e_b <= FIELD_TOL
    else:                                                                   # the path with delta = 0, alone: a record with frac = [0] and one without give the same bytes
        one = SimpleNamespace(**{k: (v[1:2] if isinstance(v, np.ndarray) and v.ndim == 1 else v) for k, v in vars(s.paths).items()})
        one.txSteering, one.rxSteering = s.paths.txSteering[1:2], s.paths.rxSteering[:, 1:2]
        assert one.frac[0] == 0.0
        with_frac = pkg.sensing.multiStaticSensing(d_waves, dims, s.carrier, s.rp, one, nfft=s.nfft, ctx=ctx, spectral_noise=np.zeros(dims)).numpy()
        del one.frac
        without = pkg.sensing.multiStaticSensing(d_waves, dims, s.carrier, s.rp, one, nfft=s.nfft, ctx=ctx, spectral_noise=np.zeros(dims)).numpy()
        assert _b(with_frac) == _b(without)


FRAC_REFUSALS = {"time_none": ("UNSUPPORTED", "NOISE_NONE", (0.37, 0.5, 0.9)), "time_injected": ("UNSUPPORTED", "NOISE_INJECTED", (0.37, 0.5, 0.9)),
                 "time_philox": ("UNSUPPORTED", "NOISE_PHILOX", (0.0, 0.0, 0.25)), "frac_one": ("INVALID_ARG", "NOISE_PHILOX_SPECTRAL", (0.0, 1.0, 0.0)),
                 "frac_negative": ("INVALID_ARG", "NOISE_PHILOX_SPECTRAL", (-1e-9, 0.5, 0.0)), "frac_nan": ("INVALID_ARG", "NOISE_INJECTED_SPECTRAL", (0.0, 0.5, np.nan)),
                 "frac_inf": ("INVALID_ARG", "NOISE_NONE", (np.inf, 0.0, 0.0))}


@pytest.mark.parametrize("name", list(FRAC_REFUSALS))
def test_refused_fractional_calls_write_nothing(pkg, ctx, name):
    status, mode, frac = FRAC_REFUSALS[name]
    L = pkg._lib
    code = {v: k for k, v in L.STATUS_NAMES.items()}[status]
    s = S.frac_scene("still")
    d_waves = [ctx.to_device(w) for w in s.waves]
    dims = (s.K, s.L, s.A)
    out = ctx.to_device(np.full(dims, POISON + 1j * POISON, dtype=np.complex128, order="F"))
    d_noise = ctx.to_device(np.zeros((s.T, s.A) if mode == "NOISE_INJECTED" else dims, dtype=np.complex128, order="F"))
    st, lo = _frac_call(pkg, ctx, s, np.array(frac), getattr(L, mode), d_noise, 5, d_waves, out)
    msg = (ctx.lib.isac_last_error(ctx.handle) or b"").decode()
    print(f"{name}: status {st} ({msg})")
    got = out.numpy()
    assert st == code and lo == -5 and (got.real == POISON).all() and (got.imag == POISON).all()


def test_python_mirror_of_the_fractional_paths(pkg, ctx):
    """multiStaticChannel returns a waveform and refuses a record with fractions; multiStaticSensing in a time-domain mode raises UNSUPPORTED."""
    s = S.frac_scene("still")
    d_waves = [ctx.to_device(w) for w in s.waves]
    with pytest.raises(ValueError):
        pkg.sensing.channelModels.multiStaticChannel(d_waves, s.rp, s.paths, ctx=ctx)
    with pytest.raises(pkg.IsacError) as e:
        pkg.sensing.multiStaticSensing(d_waves, (s.K, s.L, s.A), s.carrier, s.rp, s.paths, nfft=s.nfft, ctx=ctx, seed=3)
    assert e.value.name == "UNSUPPORTED"


# ---------------------------------------------------------------- 6
def test_end_to_end_range_between_the_bins(pkg):
    """Measured on the MI355X: refined ranges off by 1.7e-3 and 1.6e-2 bin (0.017 m and 0.156 m at rRes 9.76 m), the list's own by 0.37 and 0.39 bin; the restated chain
    (tests/test_subsample_cpu.py, another noise draw, the grid column's nu0) is off by 3.3e-4 and 1.9e-2 bin, so the two bounds stand at 0.1 and 0.05."""
    v = _e2e(pkg)
    r_res = float(v.rp.rRes)
    truth = np.array(sorted(S.E2E_BINS))
    assert np.array_equal(v.paths.shift + 1, v.ceil.shift) and np.allclose(v.paths.shift + v.paths.frac, truth, rtol=0, atol=1e-9)
    rr, fine = v.rr, v.fine
    keep = fine["sidelobe_of"] < 0
    err = np.array([np.abs(truth - r / r_res).min() for r in rr["rng"]])
    err_grid = np.array([np.abs(truth - r / r_res).min() for r in fine["rng"]])
    print(f"end to end: rows {rr['row'].tolist()}, nu {rr['nu'].tolist()}, sidelobe_of {fine['sidelobe_of'].tolist()}, status {rr['range_status'].tolist()}: rho "
          f"{rr['rho'].tolist()} for {truth.tolist()}: errors {err.tolist()} bin, the list's own {err_grid.tolist()} bin; rngRMSE {v.rmse.rngRMSE.tolist()} m (grid "
          f"{v.rmse_grid.rngRMSE.tolist()} m), rRes {r_res:.4f} m")
    assert keep.sum() >= 2 and len({int(np.abs(truth - r / r_res).argmin()) for r in rr["rng"][keep]}) == 2      # both targets are listed
    assert (rr["range_status"] == 0).all()
    assert (err <= E2E_BOUND).all()
    assert (err_grid > 0.3).all()
    assert np.array_equal(rr["rng"], rr["rho"] * r_res) and np.array_equal(rr["rng_grid"], fine["rng"]) and rr["range_snapshots"].shape == (v.sc.A, rr["rng"].size)
    for k in fine:                                                          # a copy of the list with rng replaced
        if k != "rng":
            assert np.asarray(rr[k]).tobytes() == np.asarray(fine[k]).tobytes(), k
    assert np.allclose(v.rmse.rngRMSE, err * r_res, rtol=0, atol=1e-9) and (v.rmse.rngRMSE <= E2E_BOUND * r_res).all() and (v.rmse_grid.rngRMSE > 0.3 * r_res).all()
