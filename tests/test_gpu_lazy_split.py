"""The SPLIT covariance of a native lazy echo grid (ISAC_LAZY_COV_SPLIT, the default; include/isac_lazy_cov.h): the noise term W W' formed at the head of the fused call beside
the beam-sum (cov_noise_beam_kernel), the cross term in the range kernel (echo_range_xc_kernel), the coefficient vectors from the stored beam-sums (coef_window_kernel), Ra
assembled in fft2D (cov_assemble_kernel) -- against route 1 (beamsum_coef_kernel + cov_lazy_kernel) of the same library and against the array form (the materialising
sequence of the same calls).  nIFFT 4096 at 30 kHz throughout.

  shapes   24 PRB x 14 symbols    one half-block only; the beam units far outlast the two slab steps of a workgroup: every unit goes through the tail loop
           106 PRB x 14           the partner half of the last block pair is masked (K = 1272)
           273 PRB x 14, x 28     the bench column
           each at 49 and 64 antennas (the fourth 16-block half padded / full; 9 and 11 slab steps per beam unit), one and two LoS targets (two: the range kernel is the
           plain lazy one and the cross term comes from cov_cross_kernel in fft2D)
  a scene with a zero-filled symbol range (the range kernel's early-out behind the cross term's store)
  asserted the materialised grid bit-equal between the routes and to the array the non-lazy call stores (so D, the steering table and the coefficient vectors are the same
           bits: the grid is D a + sig w); the |rdm|^2 window bit-equal (the range rows); every antenna's CFAR list and every estimate identical;
           Ra <= 1e-13 of the array form (the project's bound for another summation order, tests/test_gpu_lazy_echo.py) and exactly Hermitian, on both routes;
           that each lazy run took the route it was set to (isac_ctx_get_lazy_cov_route_used): a silent fall-back to the other route fails the test
  oracle   tests/_lazy_cpi_reference.py's independent field and covariance (comparison (B) of test_gpu_lazy_oracle.py) on BOTH routes: the default-route run there no
           longer reaches cov_lazy_kernel.
"""
from __future__ import annotations

from importlib import import_module

import numpy as np
import pytest

import _lazy_cpi_reference as R
from conftest import load_pkg

pytestmark = pytest.mark.gpu

TARGETS = {1: ((R.NEAR,), (7.0,)), 2: ((R.NEAR, R.MID), (10.0, -6.0))}


def _scene(pkg, nrb, n_sym, n_ants, q, silent=()):
    """tests/_lazy_cpi_reference.py's scene builder: the carrier at Nfft = nIFFT = 4096 whatever the PRB count (a 24-PRB carrier of its own would take a 512-point transform
    and leave the native lazy route)."""
    tg, vel = TARGETS[q]
    case = R._case(f"k{12 * nrb}_l{n_sym}_a{n_ants}_q{q}", nrb, n_ants, tg, vel, (1,) * q, n_sym, silent=silent, grid_seed=1000 + nrb + n_ants + q,
                   noise_seed=0xC0 + nrb + 3 * n_ants + q, pfa=R.pfa_for(nrb))
    return R.build_scene(case, pkg.sensing.radarParams)


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def _fft2d(pkg, rp, cf, grid, d_txg, ctx):
    dbg_fn = import_module(pkg.__name__ + ".sensing.estimation.fft2D").fft2D_debug
    try:
        return pkg.sensing.estimation.fft2D(rp, cf, grid, d_txg, return_debug=True, reuse_range=True)
    except pkg.IsacError as e:
        assert e.name == "NO_DETECTION"
        return None, dbg_fn(ctx, grid.shape[2])


def _cpi(pkg, sc, seed, route):
    """route None: the materialising sequence (the array form); 0 / 1: the lazy sequence on that covariance route.  -> (est | None, debug, grid as a NumPy array)"""
    ctx = pkg.Context()
    try:
        if route is not None:
            ctx.set_lazy_cov_route(route)
        rp = sc.rp
        cf = pkg.sensing.detection.cfar2D(rp)
        d_wave, d_txg = ctx.to_device(sc.tx_wave), ctx.to_device(sc.tx_grid)
        g = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, nfft=4096, fuse_fft2d=(rp, cf, d_txg), ctx=ctx, lazy=route is not None,
                                          seed=seed, noise_domain="spectral")
        est, dbg = _fft2d(pkg, rp, cf, g, d_txg, ctx)
        if route is not None:
            assert ctx.lazy_cov_route_used() == route, "the covariance did not take the route it was set to"
        return est, dbg, g.numpy()
    finally:
        ctx.close()


def _same_lists(a, b):
    (est_a, dbg_a), (est_b, dbg_b) = a, b
    assert np.array_equal(dbg_a.power_window, dbg_b.power_window)
    assert all(np.array_equal(x, y) for x, y in zip(dbg_a.detections, dbg_b.detections))
    assert (est_a is None) == (est_b is None)
    if est_a is not None:
        assert np.array_equal(est_a.rngEst, est_b.rngEst) and np.array_equal(est_a.velEst, est_b.velEst) and np.array_equal(est_a.aziEst, est_b.aziEst)


def _check(pkg, sc, record_property):
    seed = sc.case.noise_seed
    est_a, dbg_a, g_a = _cpi(pkg, sc, seed, None)
    est_0, dbg_0, g_0 = _cpi(pkg, sc, seed, 0)
    est_1, dbg_1, g_1 = _cpi(pkg, sc, seed, 1)
    assert np.array_equal(g_0, g_1) and np.array_equal(g_0, g_a)
    _same_lists((est_0, dbg_0), (est_1, dbg_1))
    _same_lists((est_0, dbg_0), (est_a, dbg_a))
    e0, e1 = rel(dbg_0.Ra, dbg_a.Ra), rel(dbg_1.Ra, dbg_a.Ra)
    record_property("ra_split_vs_array", e0)
    record_property("ra_regenerating_vs_array", e1)
    print(f"Ra against the array form: split {e0:.3e}, regenerating {e1:.3e}")
    assert e0 <= 1e-13 and e1 <= 1e-13
    assert np.array_equal(dbg_0.Ra, dbg_0.Ra.conj().T) and np.array_equal(dbg_1.Ra, dbg_1.Ra.conj().T)


@pytest.mark.parametrize("q", [1, 2])
@pytest.mark.parametrize("n_ants", [49, 64])
@pytest.mark.parametrize("nrb,n_sym", [(24, 14), (106, 14), (273, 14), (273, 28)])
def test_split_route_matches_route_1_and_the_array_form(pkg, nrb, n_sym, n_ants, q, record_property):
    _check(pkg, _scene(pkg, nrb, n_sym, n_ants, q), record_property)


def test_split_route_with_a_zero_filled_symbol_range(pkg, record_property):
    """Symbols 4..8 of the transmit grid are zero (an 'S' slot inside the CPI): their columns leave the range kernel early -- behind the cross term's store, which still
    counts (the echo of a silent symbol is the noise plus the tail of the delayed waveform)."""
    _check(pkg, _scene(pkg, 273, 14, 64, 1, silent=(4, 5, 6, 7, 8)), record_property)


@pytest.mark.parametrize("route", [0, 1])
@pytest.mark.parametrize("name", ["k288_a64", "k1032_a56_q2_27of28"])
def test_both_routes_against_the_independent_reference(pkg, name, route, record_property):
    """Comparison (B) of tests/test_gpu_lazy_oracle.py -- grid and Ra against the oracle's time-domain chain fed the restated Philox field, every bound from the reference --
    with the covariance route set explicitly."""
    case = next(c for c in R.TABLE if c.name == name)
    sc, e, ra_ref, m, eta = R.reference_of(case, pkg.sensing.radarParams)
    ctx = pkg.Context()
    try:
        ctx.set_lazy_cov_route(route)
        cf = pkg.sensing.detection.cfar2D(sc.rp)
        d_wave, d_txg = ctx.to_device(sc.tx_wave), ctx.to_device(sc.tx_grid)
        lz = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, sc.rp, sc.los, nfft=4096, ctx=ctx, lazy=True, fuse_fft2d=(sc.rp, cf, d_txg),
                                           seed=sc.case.noise_seed, noise_domain="spectral")
        _, dbg = _fft2d(pkg, sc.rp, cf, lz, d_txg, ctx)
        assert ctx.lazy_cov_route_used() == route
        g = lz.numpy()
    finally:
        ctx.close()
    e_err = float(np.abs(g - e).max())
    r_err = float((np.abs(dbg.Ra - ra_ref) / R.covariance_bound(eta, m, ra_ref)).max())
    record_property("echo_err_over_eta", e_err / eta)
    record_property("ra_err_over_bound", r_err)
    print(f"{name} route {route}: |g - E| {e_err / eta:.3f} eta; Ra error {r_err:.3f} of its bound")
    assert e_err <= eta and r_err <= 1.0
    assert np.array_equal(dbg.Ra, dbg.Ra.conj().T)
