"""The echo chain and fft2D on physical scenes at 15, 60 and 120 kHz, against the oracle.  The library takes the numerology from the carrier (csrc/ofdm_symbol.hpp: long prefix
every 7 * 2^mu symbols, cp_base + 16 (Nfft / 2048) 2^mu samples long); every other physical scene of the suite is at 30 kHz, where a kernel that assumed "long prefix every 14
symbols" or a wrapper that passed 30 for the carrier's spacing would go unnoticed.  The scenes (tests/_numerology_scenes.py; the checker itself: tests/test_numerology_cpu.py)
also put target delays beyond the cyclic prefix -- at 120 kHz up to 217 samples against a 72-sample prefix -- so that the previous symbol's echo lies inside the window.

RTOL = 1e-10 relative to the field's maximum (test_gpu_parity.py, test_gpu_spectral.py); the oracle and the C++ port agree to 1.7e-14 on these scenes.  Lists and estimates are
compared exactly, after asserting that no CUT cell lies within 1e-6 (relative) of its threshold.  Every comparison records its measured error (record_property).

  (a) echo grid with time-domain noise, all eight scenes, host and device arrays; one 120 kHz scene with a cut waveform and a padded symbol dimension
  (b) the spectral noise modes against the oracle's time-domain chain (conftest.spectral_to_time_noise at the carrier's spacing)
  (c) fft2D: |rdm|^2 window, Ra, CFAR lists, estimates -- on the oracle's grid, on the device's own, with ISAC_OPT_TAIL_FUSION 0 and 1
  (d) the fused route (Nfft = nIFFT = 4096, K = 288) at 15 / 60 / 120 kHz: symbol counts on both sides of the second long prefix, delays around both prefix lengths; bit for bit
      the reference route, which is itself anchored to the oracle at Nfft = 4096 per spacing
  (e) the lazy echo grid at 15 and 120 kHz (49 antennas), both lazy covariance routes; one 120 kHz lazy CPI against tests/_lazy_cpi_reference.py"""
from __future__ import annotations

import ctypes as C
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest

import oracle as O
import _lazy_cpi_reference as R
import _numerology_scenes as N
from conftest import load_pkg, spectral_to_time_noise

pytestmark = pytest.mark.gpu
RTOL = 1e-10
MARGIN = 1e-6
LIGHTSPEED = 299792458.0
HOST_ARRAYS = ("scs15_nrb24_a4", "scs60_nrb11_a2")                          # (a) through the host-pointer entry point; every other scene through DeviceArrays
SPECTRAL = ("scs15_nrb24_a4", "scs60_nrb66_a3", "scs120_nrb24_a4", "scs120_nrb66_a3")      # the table's rows 1, 4, 5, 6
OWN_GRID = ("scs60_nrb24_a4", "scs120_nrb66_a3")                            # rows 3 and 6
TAIL = "scs120_nrb66_a3"                                                    # row 6
PARTIAL = "scs120_nrb11_a2"


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def _bits(x):
    return np.ascontiguousarray(np.asarray(x).ravel(order="K")).view(np.uint64)


def _unit_noise(shape, seed):
    rng = np.random.default_rng(seed)
    return np.asfortranarray(rng.standard_normal(shape) + 1j * rng.standard_normal(shape))


def _lib_params(pkg, sc):
    rp = pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)
    return rp, pkg.sensing.detection.cfar2D(rp)


_device_echo = {}


def _echo_on_device(pkg, case):
    """The library's echo grid of a table scene with the scene's time-domain noise, as a NumPy array: run once per process, read-only."""
    if case.name not in _device_echo:
        sc = N.oracle_of(case).sc
        rp, _ = _lib_params(pkg, sc)
        if case.name in HOST_ARRAYS:
            got = pkg.sensing.monoStaticSensing(sc.tx_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft)
        else:
            ctx = pkg.default_context()
            got = pkg.sensing.monoStaticSensing(ctx.to_device(sc.tx_wave), sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=ctx.to_device(sc.noise), nfft=sc.wave.Nfft).numpy()
        got = np.asfortranarray(got)
        got.setflags(write=False)
        _device_echo[case.name] = got
    return _device_echo[case.name]


# ---------------------------------------------------------------- (a) echo grid, time-domain noise
@pytest.mark.parametrize("case", N.CASES, ids=lambda c: c.name)
def test_echo_grid_with_time_domain_noise(pkg, case, record_property):
    o = N.oracle_of(case)
    got = _echo_on_device(pkg, case)
    err = N.rel(got, o.echo)
    record_property("echo_rel", err)
    print(f"(a) {case.name}: echo grid rel {err:.3e}")
    assert got.shape == o.echo.shape == (12 * case.nrb, case.L, case.n_ants) and err < RTOL


def test_echo_grid_of_a_cut_waveform_with_padded_symbols(pkg, record_property):
    """120 kHz, the waveform 7 samples short (the last symbol incomplete) and txDimension(2) = L + 6: monoStaticSensing.m:19-21 pads with zero columns."""
    case = N.CASE[PARTIAL]
    sc = N.oracle_of(case).sc
    rp, _ = _lib_params(pkg, sc)
    wave, noise = np.asfortranarray(sc.tx_wave[:-7]), np.asfortranarray(sc.noise[:-7])
    shape = (sc.K, sc.L + 6, sc.A)
    want = O.mono_static_sensing(wave, shape, sc.carrier, sc.rp, sc.los, noise, nfft=sc.wave.Nfft)
    ctx = pkg.default_context()
    got = pkg.sensing.monoStaticSensing(ctx.to_device(wave), shape, sc.carrier, rp, sc.los, noise=ctx.to_device(noise), nfft=sc.wave.Nfft).numpy()
    err = N.rel(got[:, :sc.L - 1, :], want[:, :sc.L - 1, :])
    record_property("echo_rel", err)
    print(f"(a) {case.name}, cut waveform: echo grid rel {err:.3e}")
    assert got.shape == want.shape == shape and not want[:, sc.L - 1:, :].any() and want[:, sc.L - 2, :].any()
    assert np.all(got[:, sc.L - 1:, :] == 0) and err < RTOL and N.rel(got, want) < RTOL


# ---------------------------------------------------------------- (b) spectral noise modes
@pytest.mark.parametrize("name", SPECTRAL)
def test_spectral_noise_modes_match_the_time_domain_oracle(pkg, name, record_property):
    case = N.CASE[name]
    sc = N.oracle_of(case).sc
    rp, _ = _lib_params(pkg, sc)
    nfft, shape = sc.wave.Nfft, sc.tx_grid.shape
    w = _unit_noise(shape, case.nrb + case.n_ants + case.scs)
    tnoise = spectral_to_time_noise(w, sc.T, nfft, case.scs, sc.rp.fc, sc.rp.fs)
    want = O.mono_static_sensing(sc.tx_wave, shape, sc.carrier, sc.rp, sc.los, tnoise, nfft=nfft)
    got = pkg.sensing.monoStaticSensing(sc.tx_wave, shape, sc.carrier, rp, sc.los, spectral_noise=w, nfft=nfft)
    want0 = O.mono_static_sensing(sc.tx_wave, shape, sc.carrier, sc.rp, sc.los, None, nfft=nfft)
    got0 = pkg.sensing.monoStaticSensing(sc.tx_wave, shape, sc.carrier, rp, sc.los, spectral_noise=np.zeros_like(w), nfft=nfft)
    got_t = pkg.sensing.monoStaticSensing(sc.tx_wave, shape, sc.carrier, rp, sc.los, noise=tnoise, nfft=nfft)
    errs = dict(injected_rel=N.rel(got, want), noiseless_rel=N.rel(got0, want0), own_time_route_rel=N.rel(got, got_t))
    for k, v in errs.items():
        record_property(k, v)
    print(f"(b) {name}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert got.shape == want.shape
    assert errs["injected_rel"] < RTOL                                      # HIP(spectral W) == oracle(the time-domain noise that demodulates to W)
    assert errs["noiseless_rel"] < RTOL                                     # the factorisation sum_q a_q D_q alone against the per-antenna demodulation
    assert errs["own_time_route_rel"] < RTOL                                # ... and against the library's own time-domain kernels
    assert float(np.abs(want - want0).max()) > RTOL * float(np.abs(want0).max())                      # the noise is there: the first comparison is not the second


# ---------------------------------------------------------------- (c) fft2D
def _check_fft2d(o, got, gd, record_property, what):
    """test_gpu_parity._run_fft2d_case's assertions against the oracle's fft2D on the oracle's grid; the guard margin first."""
    sc = o.sc
    assert all(m >= MARGIN for m in o.margin), f"scene too close to a threshold: {min(o.margin):.2e}"
    r0, c0 = gd.first_row - 1, gd.first_col - 1
    nr, nc, na = gd.power_window.shape
    w_err = N.rel(gd.power_window, np.abs(o.dbg.rdm[r0:r0 + nr, c0:c0 + nc, :]) ** 2)
    ra_err = N.rel(gd.Ra, o.dbg.Ra)
    record_property(what + "_window_rel", w_err)
    record_property(what + "_ra_rel", ra_err)
    print(f"(c) {what}: |rdm|^2 window rel {w_err:.3e}, Ra rel {ra_err:.3e}, guard margin {min(o.margin):.2e}")
    assert na == sc.A and w_err < RTOL
    assert ra_err < RTOL and np.array_equal(gd.Ra, gd.Ra.conj().T)
    assert len(gd.detections) == sc.A
    for a in range(sc.A):
        assert np.array_equal(gd.detections[a], o.dbg.detections[a]), f"antenna {a}"
    assert np.array_equal(got.rngEst, o.est.rngEst) and np.array_equal(got.velEst, o.est.velEst)
    assert np.array_equal(got.aziEst, o.est.aziEst) and np.isnan(got.eleEst).all() and got.rngEst.size >= 1


@pytest.mark.parametrize("case", N.CASES, ids=lambda c: c.name)
def test_fft2d_on_the_oracle_grid(pkg, case, record_property):
    o = N.oracle_of(case)
    rp, cf = _lib_params(pkg, o.sc)
    got, gd = pkg.sensing.estimation.fft2D(rp, cf, o.echo, o.sc.tx_grid, return_debug=True)
    _check_fft2d(o, got, gd, record_property, case.name)


@pytest.mark.parametrize("name", OWN_GRID)
def test_fft2d_on_the_device_grid(pkg, name, record_property):
    """The grid fft2D consumes is the echo path's own output (within RTOL of the oracle's, (a)); lists and estimates are still the oracle's."""
    case = N.CASE[name]
    o = N.oracle_of(case)
    rx = _echo_on_device(pkg, case)
    assert N.rel(rx, o.echo) < RTOL
    rp, cf = _lib_params(pkg, o.sc)
    ctx = pkg.default_context()
    got, gd = pkg.sensing.estimation.fft2D(rp, cf, ctx.to_device(rx), ctx.to_device(o.sc.tx_grid), return_debug=True)
    _check_fft2d(o, got, gd, record_property, name + "_own_grid")


@pytest.mark.parametrize("fused", [False, True], ids=["tail_fusion_0", "tail_fusion_1"])
def test_fft2d_with_both_detector_tails(pkg, fused, record_property):
    case = N.CASE[TAIL]
    o = N.oracle_of(case)
    rp, cf = _lib_params(pkg, o.sc)
    ctx = pkg.Context()
    try:
        ctx.set_tail_fusion(fused)
        got, gd = pkg.sensing.estimation.fft2D(rp, cf, ctx.to_device(o.echo), ctx.to_device(o.sc.tx_grid), return_debug=True)
    finally:
        ctx.close()
    _check_fft2d(o, got, gd, record_property, f"{TAIL}_tail_fusion_{int(fused)}")


# ---------------------------------------------------------------- (d) the fused route off 30 kHz
def _cp(scs):
    base, long_ = (int(v) for v in O.cp_lengths(4096, scs, 2)[::-1])
    return base, long_


def _fused_scene(pkg, ctx, scs, n_ants, n_sym, delays, seed):
    """test_gpu_beam_window._scene with the spacing as a parameter: a random [T x A] transmit waveform of n_sym whole symbols + 37 samples, a QPSK transmit grid for the range
    stage, Nfft = nIFFT = 4096 at K = 288, and targets that sit at the given delays exactly: range = (d - 1/2) c Ts / 2, so ceil(pathDelay / Ts) = d."""
    ci = SimpleNamespace(NRBsDL=24, SubcarrierSpacing=scs)
    wi = SimpleNamespace(Nfft=4096, SampleRate=4096 * scs * 1e3, SymbolsPerSlot=14, SlotsPerSubframe=scs // 15)
    q = len(delays)
    cell = O.default_cell_params(n_ants=n_ants, target_pos=tuple((100.0 + 40.0 * i, 20.0 - 30.0 * i, 1.5) for i in range(q)), velocity=tuple(7.0 - 10.0 * i for i in range(q)))
    rp = pkg.sensing.radarParams(cell, ci, wi)
    rp.nIFFT = 4096
    rp.rRes = LIGHTSPEED / (2 * scs * 1e3 * rp.nIFFT)
    rp.range = np.array([max(d - 0.5, 0.0) * LIGHTSPEED / (2.0 * rp.fs) for d in delays])
    assert N.delays_of(rp) == tuple(delays)
    car = pkg._lib.Carrier(288, 4096, scs, 0)
    t = C.c_int64(0)
    assert ctx.lib.isac_ofdm_waveform_length(C.byref(car), C.c_int32(n_sym), C.byref(t)) == 0
    assert int(t.value) == int(O.symbol_starts(4096, scs, n_sym + 1)[0][n_sym])
    T = int(t.value) + 37
    rng = np.random.default_rng(seed)
    wave = np.asfortranarray(rng.standard_normal((T, n_ants)) + 1j * rng.standard_normal((T, n_ants)))
    bits = rng.integers(0, 2, (2, 288, n_sym, n_ants)) * 2 - 1
    tx_grid = np.asfortranarray((bits[0] + 1j * bits[1]) / np.sqrt(2.0))
    return SimpleNamespace(carrier=ci, rp=rp, cf=pkg.sensing.detection.cfar2D(rp), los=np.ones(q, dtype=np.uint8), shape=tx_grid.shape,
                           d_wave=ctx.to_device(wave), d_txg=ctx.to_device(tx_grid))


def _fft2d(pkg, ctx, sc, grid, reuse):
    """(est | None, debug): a scene without a CFAR detection raises NO_DETECTION on every route alike; window, lists and Ra are still there to compare."""
    try:
        return pkg.sensing.estimation.fft2D(sc.rp, sc.cf, grid, sc.d_txg, return_debug=True, reuse_range=reuse)
    except pkg.IsacError as e:
        assert e.name == "NO_DETECTION"
        return None, import_module(pkg.__name__ + ".sensing.estimation.fft2D").fft2D_debug(ctx, grid.shape[2])


def _same_lists(a, b, what):
    (est_a, dbg_a), (est_b, dbg_b) = a, b
    pa, pb = np.asarray(dbg_a.power_window), np.asarray(dbg_b.power_window)
    assert pa.shape == pb.shape and pa.tobytes(order="F") == pb.tobytes(order="F"), what + ": |rdm|^2 window"
    assert len(dbg_a.detections) == len(dbg_b.detections) and all(np.array_equal(x, y) for x, y in zip(dbg_a.detections, dbg_b.detections)), what + ": CFAR lists"
    assert (est_a is None) == (est_b is None), what
    if est_a is not None:
        assert np.array_equal(est_a.rngEst, est_b.rngEst) and np.array_equal(est_a.velEst, est_b.velEst) and np.array_equal(est_a.aziEst, est_b.aziEst), what + ": estimates"


def _fused_against_reference_route(pkg, ctx, sc, **noise):
    kw = dict(nfft=4096, ctx=ctx, **noise)
    ref = pkg.sensing.monoStaticSensing(sc.d_wave, sc.shape, sc.carrier, sc.rp, sc.los, **kw)
    r_ref = _fft2d(pkg, ctx, sc, ref, False)
    g_ref = ref.numpy()
    fused = pkg.sensing.monoStaticSensing(sc.d_wave, sc.shape, sc.carrier, sc.rp, sc.los, fuse_fft2d=(sc.rp, sc.cf, sc.d_txg), **kw)
    r_fused = _fft2d(pkg, ctx, sc, fused, True)
    g_fused = fused.numpy()
    assert g_fused.shape == g_ref.shape == sc.shape and g_ref.any()
    assert np.array_equal(_bits(g_fused), _bits(g_ref)), "echo grid: fused entry point vs isac_mono_static_sensing_dev"
    _same_lists(r_ref, r_fused, "fft2D(reuse_range=True) vs the unfused pair")
    return g_ref


def _fused_cases(scs):
    base, long_ = _cp(scs)
    edges = N.LONG_CP_EDGES[scs]
    delays = [(base // 2,), (base,), (long_,), (long_ + 1,), (2 * long_,), (1, long_ + base)]          # the pair: d_max - d_min > cp_long
    return [pytest.param(scs, 2 + i % 2, edges[i % len(edges)], d, id=f"scs{scs}_a{2 + i % 2}_l{edges[i % len(edges)]}_d{'_'.join(str(v) for v in d)}") for i, d in enumerate(delays)]


@pytest.mark.parametrize("scs,n_ants,n_sym,delays", _fused_cases(15) + _fused_cases(60) + _fused_cases(120))
def test_fused_route_matches_the_reference_route(pkg, scs, n_ants, n_sym, delays):
    ctx = pkg.Context()
    try:
        sc = _fused_scene(pkg, ctx, scs, n_ants, n_sym, delays, seed=1000 * n_sym + sum(delays) + scs)
        zeros = ctx.to_device(np.zeros(sc.shape, dtype=np.complex128, order="F"))
        g0 = _fused_against_reference_route(pkg, ctx, sc, spectral_noise=zeros)
        g1 = _fused_against_reference_route(pkg, ctx, sc, seed=0xBEA0 + n_sym + scs, noise_domain="spectral")
        assert not np.array_equal(g0, g1)
    finally:
        ctx.close()


def test_fused_cases_reach_every_edge():
    for scs in (15, 60, 120):
        ps = [p.values for p in _fused_cases(scs)]
        base, long_ = _cp(scs)
        assert (base, long_) == (288, 288 + 32 * scs // 15)
        assert {p[2] for p in ps} == set(N.LONG_CP_EDGES[scs]) and {p[1] for p in ps} == {2, 3}
        assert {p[3] for p in ps if len(p[3]) == 1} == {(base // 2,), (base,), (long_,), (long_ + 1,), (2 * long_,)}
        assert sum(len(p[3]) == 2 and max(p[3]) - min(p[3]) > long_ for p in ps) == 1


@pytest.mark.parametrize("scs,n_ants,n_slots", [(15, 3, 2), (60, 2, 3), (120, 2, 5)])
def test_reference_route_at_4096_matches_the_oracle(pkg, scs, n_ants, n_slots, record_property):
    """The anchor of (d): a modulated QPSK waveform at Nfft = 4096 forced on both sides (24 PRB), two targets, a CPI that crosses the numerology's second long prefix: the
    reference route (isac_mono_static_sensing_dev, injected spectral noise) against the oracle's time-domain chain; the fused entry point stores the same bits."""
    sc = N.scene(scs, 24, n_ants, n_slots, N.PAIR, (10.0, -6.0), n_slots + 2, False, seed=3, with_noise=False, nfft=4096)
    assert sc.wave.Nfft == 4096 and sc.rp.fs == 4096 * scs * 1e3 and sc.L > 7 * scs // 15 and sc.T == int(O.symbol_starts(4096, scs, sc.L + 1)[0][sc.L])
    rp, _ = _lib_params(pkg, sc)
    rp.nIFFT = 4096
    rp.rRes = LIGHTSPEED / (2 * scs * 1e3 * rp.nIFFT)
    cf = pkg.sensing.detection.cfar2D(rp)
    shape = sc.tx_grid.shape
    w = _unit_noise(shape, 40 + scs)
    want = O.mono_static_sensing(sc.tx_wave, shape, sc.carrier, sc.rp, sc.los, spectral_to_time_noise(w, sc.T, 4096, scs, sc.rp.fc, sc.rp.fs), nfft=4096)
    ctx = pkg.Context()
    try:
        d_wave, d_txg, d_w = ctx.to_device(sc.tx_wave), ctx.to_device(sc.tx_grid), ctx.to_device(w)
        ref = pkg.sensing.monoStaticSensing(d_wave, shape, sc.carrier, rp, sc.los, nfft=4096, ctx=ctx, spectral_noise=d_w).numpy()
        fused = pkg.sensing.monoStaticSensing(d_wave, shape, sc.carrier, rp, sc.los, nfft=4096, ctx=ctx, spectral_noise=d_w, fuse_fft2d=(rp, cf, d_txg)).numpy()
    finally:
        ctx.close()
    err = N.rel(ref, want)
    record_property("echo_rel", err)
    print(f"(d) scs {scs}: reference route at Nfft 4096 against the oracle, rel {err:.3e}; delays {N.delays_of(sc.rp)}")
    assert ref.shape == want.shape and err < RTOL
    assert np.array_equal(_bits(fused), _bits(ref))


# ---------------------------------------------------------------- (e) the lazy grid
@pytest.mark.parametrize("scs", [15, 120])
def test_lazy_grid_off_30_khz(pkg, scs, record_property):
    """49 antennas (the smallest natively lazy count), K = 288, two targets, Philox spectral noise, a symbol count just past the second long prefix: the lazy call materialises
    to the reference route's bytes; the cached fft2D on it gives the lists and estimates of fft2D on the stored grid; Ra within the 1e-13 include/isac.h states, on both routes."""
    base, long_ = _cp(scs)
    n_sym = N.LONG_CP_EDGES[scs][2]
    delays = (base // 2 - 58, base + long_ + 47)                            # d_max - d_min > cp_long
    assert delays[1] - delays[0] > long_
    runs = {}
    for route in (None, 0, 1):                                              # None: the reference route and plain fft2D on the grid it stored
        ctx = pkg.Context()
        try:
            sc = _fused_scene(pkg, ctx, scs, 49, n_sym, delays, seed=4900 + scs)
            kw = dict(nfft=4096, ctx=ctx, seed=0x1A2B + scs, noise_domain="spectral")
            if route is None:
                g = pkg.sensing.monoStaticSensing(sc.d_wave, sc.shape, sc.carrier, sc.rp, sc.los, **kw)
                res = _fft2d(pkg, ctx, sc, g, False)
            else:
                ctx.set_lazy_cov_route(route)
                g = pkg.sensing.monoStaticSensing(sc.d_wave, sc.shape, sc.carrier, sc.rp, sc.los, fuse_fft2d=(sc.rp, sc.cf, sc.d_txg), lazy=True, **kw)
                assert g.shape == sc.shape
                res = _fft2d(pkg, ctx, sc, g, True)
                assert ctx.lazy_cov_route_used() == route, "the covariance did not take the route it was set to"
            runs[route] = (res, g.numpy())
        finally:
            ctx.close()
    (r_ref, g_ref) = runs[None]
    assert g_ref.shape == (288, n_sym, 49) and g_ref.any()
    for route in (0, 1):
        r_lz, g_lz = runs[route]
        assert np.array_equal(_bits(g_lz), _bits(g_ref)), f"route {route}: materialised lazy grid vs isac_mono_static_sensing_dev"
        _same_lists(r_ref, r_lz, f"route {route}: cached fft2D on the lazy grid vs fft2D on the stored grid")
        err = N.rel(r_lz[1].Ra, r_ref[1].Ra)
        record_property(f"ra_route{route}_vs_array", err)
        print(f"(e) scs {scs} route {route}: Ra against the array form {err:.3e}")
        assert err <= 1e-13 and np.array_equal(r_lz[1].Ra, r_lz[1].Ra.conj().T)
    x = g_ref.reshape(-1, 49, order="F")
    assert N.rel(r_ref[1].Ra, (x.conj().T @ x) / x.shape[0]) < 1e-12       # Ra[a, b] = sum_n conj(G[n, a]) G[n, b] / N  (fft2D.m:106-107)


def test_lazy_cpi_at_120_khz_against_the_oracle(pkg, record_property):
    """tests/test_gpu_lazy_oracle.py's two comparisons, under its tolerances, on one 120 kHz CPI of 57 symbols (tests/_lazy_cpi_reference.py with the spacing as an argument):
    (B) the materialised grid and Ra against the oracle's time-domain chain fed the restated Philox field, every bound from the reference; (A) the oracle's fft2D on the
    materialised grid: |rdm|^2 window and Ra within RTOL, lists and estimates exact, after the two suitability guards."""
    case = N.lazy_cpi_case_120()
    sc, e, ra_ref, m, eta = R.reference_of(case, pkg.sensing.radarParams)
    ctx = pkg.Context()
    try:
        cf = pkg.sensing.detection.cfar2D(sc.rp)
        d_wave, d_txg = ctx.to_device(sc.tx_wave), ctx.to_device(sc.tx_grid)
        lz = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, sc.rp, sc.los, nfft=4096, ctx=ctx, lazy=True, fuse_fft2d=(sc.rp, cf, d_txg),
                                           seed=case.noise_seed, noise_domain="spectral")
        assert lz.shape == sc.tx_grid.shape
        est, dbg = pkg.sensing.estimation.fft2D(sc.rp, cf, lz, d_txg, return_debug=True, reuse_range=True)
        g = lz.numpy()
    finally:
        ctx.close()
    # (B)
    e_err = float(np.abs(g - e).max())
    r_err = float((np.abs(dbg.Ra - ra_ref) / R.covariance_bound(eta, m, ra_ref)).max())
    record_property("echo_err_over_eta", e_err / eta)
    record_property("ra_err_over_bound", r_err)
    print(f"(e) {case.name}: |g - E| {e_err / eta:.3f} eta; Ra error {r_err:.3f} of its bound; eta / max|E| {eta / float(np.abs(e).max()):.2e}")
    assert g.shape == e.shape and e_err <= eta and r_err <= 1.0
    # (A)
    o = R.oracle_chain(sc, g)
    record_property("cfar_margin", o.cfar_margin)
    record_property("eig_gap_over_w0", o.eig_gap)
    assert o.cfar_margin > 1e-7, f"unsuitable input: a CUT cell lies within {o.cfar_margin:.2e} of its threshold"
    assert o.eig_gap > 1e-9, f"unsuitable input: eigenvalue gap {o.eig_gap:.2e} w[0] at the signal / noise split"
    r0, c0 = dbg.first_row, dbg.first_col
    nr, nc, na = dbg.power_window.shape
    w_err = N.rel(dbg.power_window, np.abs(o.rdm[r0 - 1:r0 - 1 + nr, c0 - 1:c0 - 1 + nc, :]) ** 2)
    ra_err = N.rel(dbg.Ra, o.Ra)
    record_property("window_rel", w_err)
    record_property("ra_rel", ra_err)
    print(f"(e) {case.name}: |rdm|^2 window {w_err:.3e}, Ra {ra_err:.3e}; detections {o.n_det}, CFAR margin {o.cfar_margin:.2e}, eigenvalue gap {o.eig_gap:.2e} w[0]")
    assert na == sc.A and w_err < RTOL and ra_err <= RTOL and np.array_equal(dbg.Ra, dbg.Ra.conj().T)
    for a in range(sc.A):
        assert np.array_equal(dbg.detections[a], o.detections[a]), f"antenna {a}"
    assert o.est is not None and o.n_det > 0
    assert np.array_equal(est.rngEst, o.est.rngEst) and np.array_equal(est.velEst, o.est.velEst) and np.array_equal(est.aziEst, o.est.aziEst), (est, o.est)
