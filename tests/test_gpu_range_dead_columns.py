"""echo_range_xc_kernel's dead-column test (csrc/echo.hip): a column (symbol l, antenna r) with tx[., l, r] == 0 AND D[., l] == 0 and a finite sig leaves the range kernel
of the split lazy CPI before anything is drawn for it -- +0.0 to its range rows and to its cross-term entry.  The D half is a flag per symbol that the demod_kernel launch
which forms D writes; the tx half is a peek made only where that flag is set.  Every other column takes the kernel's unchanged text.

Every case runs the native lazy split route (one LoS target, spectral Philox noise, nIFFT 4096) and compares
  * the |rdm|^2 window, every antenna's CFAR list and the estimates BYTE FOR BYTE, and Ra within the suite's 1e-13 (another summation order), against the same CPI on the
    regenerating route (isac_ctx_set_lazy_cov_route(1)): echo_range_sl_kernel<1, 1, false, 4> + cov_lazy_kernel, neither of which has the test -- an independent reference;
  * Ra within 1e-13 against the array form, as tests/test_gpu_lazy_split.py does.
What kind of column a case is about is read off its INPUT, so that no case passes vacuously: tx == 0 from the transmit grid, D == 0 from a noiseless array-form run of the
same scene (N0 = 0: the stored grid is D a, bit for bit), and each case asserts that the kind exists.

  dead columns between live ones     A in {49, 64} x K in {300, 3276} (a partial last wave; rows k >= K in both parities), symbols 0, 4, 5 and 13 silent -- the first and the
                                     last column of an antenna plane among them; the echo delay (86 samples) stays inside the half prefix the demodulation window skips
  a silent 'S' slot, L = 56          symbols 42..55 zero (isac_synth_qpsk_grid_dev's zero_s_slots pattern: the fourth slot)
  tx == 0 but D != 0                 the same silent symbols with a target 216 samples away: the previous symbol's echo reaches into the silent symbol's window -- the
                                     full path must run and the cross term must count
  every column dead                  an all-zero transmit grid: rows all zero, Ra = the noise term alone
  one denormal / one NaN tx sample   in an otherwise silent column: the column is live (the compare is a floating-point one: NaN and denormals are not zero)
"""
from __future__ import annotations

import copy

import numpy as np
import pytest

import _lazy_cpi_reference as R
from conftest import load_pkg
from test_gpu_lazy_split import _fft2d, rel

pytestmark = pytest.mark.gpu

SILENT = (0, 4, 5, 13)


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def _scene(pkg, nrb, n_sym, n_ants, target=R.NEAR, silent=SILENT, zero_from=None):
    case = R._case(f"dead_k{12 * nrb}_l{n_sym}_a{n_ants}", nrb, n_ants, (target,), (7.0,), (1,), n_sym, silent=silent, zero_from=zero_from, grid_seed=2000 + nrb + n_ants,
                   noise_seed=0xD0 + nrb + 3 * n_ants, pfa=R.pfa_for(nrb))
    return R.build_scene(case, pkg.sensing.radarParams)


def _cpi(pkg, sc, tx_grid, route):
    """route None: the array form; 0: split (the kernel under test); 1: regenerating.  -> (est | None, debug)"""
    ctx = pkg.Context()
    try:
        if route is not None:
            ctx.set_lazy_cov_route(route)
        cf = pkg.sensing.detection.cfar2D(sc.rp)
        d_wave, d_txg = ctx.to_device(sc.tx_wave), ctx.to_device(tx_grid)
        g = pkg.sensing.monoStaticSensing(d_wave, tx_grid.shape, sc.carrier, sc.rp, sc.los, nfft=4096, fuse_fft2d=(sc.rp, cf, d_txg), ctx=ctx, lazy=route is not None,
                                          seed=sc.case.noise_seed, noise_domain="spectral")
        est, dbg = _fft2d(pkg, sc.rp, cf, g, d_txg, ctx)
        if route is not None:
            assert ctx.lazy_cov_route_used() == route, "the covariance did not take the route it was set to"
        return est, dbg
    finally:
        ctx.close()


def _d_times_a(pkg, sc):
    """The noiseless stored grid D a [K x L x A] (N0 = 0): a symbol's D column is zero exactly where this is zero on every antenna (|a[r]| = 1)."""
    rp0 = copy.copy(sc.rp)
    rp0.N0 = 0.0
    ctx = pkg.Context()
    try:
        g = pkg.sensing.monoStaticSensing(ctx.to_device(sc.tx_wave), sc.tx_grid.shape, sc.carrier, rp0, sc.los, nfft=4096, ctx=ctx, seed=1, noise_domain="spectral")
        return g.numpy()
    finally:
        ctx.close()


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _kinds(pkg, sc, tx_grid):
    """Per (l, r): tx column zero (floating-point compare), and per l: D column zero."""
    with np.errstate(invalid="ignore"):
        tx_zero = np.all(tx_grid == 0, axis=0)                                                  # [L x A]; NaN == 0 is False
    d_zero = np.all(_d_times_a(pkg, sc) == 0, axis=(0, 2))[:sc.L_whole]                       # [L]
    return tx_zero, d_zero


def _check(pkg, sc, tx_grid, record_property):
    (est_0, dbg_0), (est_1, dbg_1), (est_a, dbg_a) = _cpi(pkg, sc, tx_grid, 0), _cpi(pkg, sc, tx_grid, 1), _cpi(pkg, sc, tx_grid, None)
    assert _same_bytes(dbg_0.power_window, dbg_1.power_window)
    assert len(dbg_0.detections) == len(dbg_1.detections) and all(_same_bytes(x, y) for x, y in zip(dbg_0.detections, dbg_1.detections))
    assert (est_0 is None) == (est_1 is None)
    if est_0 is not None:
        assert _same_bytes(est_0.rngEst, est_1.rngEst) and _same_bytes(est_0.velEst, est_1.velEst) and _same_bytes(est_0.aziEst, est_1.aziEst)
    e1, ea = rel(dbg_0.Ra, dbg_1.Ra), rel(dbg_0.Ra, dbg_a.Ra)
    record_property("ra_split_vs_regenerating", e1)
    record_property("ra_split_vs_array", ea)
    print(f"Ra of the split route: {e1:.3e} from the regenerating route, {ea:.3e} from the array form")
    assert e1 <= 1e-13 and ea <= 1e-13
    assert np.array_equal(dbg_0.Ra, dbg_0.Ra.conj().T)
    return dbg_0


@pytest.mark.parametrize("n_ants", [49, 64])
@pytest.mark.parametrize("nrb", [25, 273])
def test_dead_columns_between_live_ones(pkg, nrb, n_ants, record_property):
    sc = _scene(pkg, nrb, 14, n_ants)
    tx_zero, d_zero = _kinds(pkg, sc, sc.tx_grid)
    dead = tx_zero & d_zero[:, None]
    assert dead[list(SILENT)].all() and dead.sum() == len(SILENT) * n_ants, "the silent symbols are dead on every antenna, the first and last column of a plane among them"
    assert not d_zero[1] and not tx_zero[1].any()
    _check(pkg, sc, sc.tx_grid, record_property)


def test_silent_slot_of_a_four_slot_cpi(pkg, record_property):
    sc = _scene(pkg, 25, 56, 64, silent=(), zero_from=42)
    tx_zero, d_zero = _kinds(pkg, sc, sc.tx_grid)
    dead = tx_zero & d_zero[:, None]
    assert dead[42:].all() and not dead[:42].any(), "one silent slot behind three live ones"
    _check(pkg, sc, sc.tx_grid, record_property)


def test_silent_column_whose_d_is_not_zero_takes_the_full_path(pkg, record_property):
    sc = _scene(pkg, 25, 14, 64, target=R.MID, silent=(4, 5))
    tx_zero, d_zero = _kinds(pkg, sc, sc.tx_grid)
    assert tx_zero[4].all() and tx_zero[5].all()
    assert not d_zero[4], "the echo of symbol 3 reaches into symbol 4's demodulation window: D[., 4] != 0"
    _check(pkg, sc, sc.tx_grid, record_property)


def test_every_column_dead(pkg, record_property):
    sc = _scene(pkg, 25, 14, 49, silent=tuple(range(14)))
    tx_zero, d_zero = _kinds(pkg, sc, sc.tx_grid)
    assert tx_zero.all() and d_zero.all()
    dbg = _check(pkg, sc, sc.tx_grid, record_property)
    assert not np.any(dbg.power_window), "every range row is zero"
    assert np.all(np.real(np.diag(dbg.Ra)) > 0), "Ra is the noise term"


@pytest.mark.parametrize("value", [5e-324, float("nan")], ids=["denormal", "nan"])
def test_one_nonzero_sample_makes_the_column_live(pkg, value, record_property):
    sc = _scene(pkg, 25, 14, 64)
    tx_grid = np.array(sc.tx_grid, order="F")
    tx_grid[299, 5, 63] = value                                                                 # the last row of a partial wave, the last antenna, a silent symbol
    tx_zero, d_zero = _kinds(pkg, sc, tx_grid)
    assert d_zero[5] and not tx_zero[5, 63] and tx_zero[5, :63].all(), "one live column in a silent symbol"
    _check(pkg, sc, tx_grid, record_property)
