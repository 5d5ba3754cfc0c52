"""The lazy CPI after the generator's instruction diet (echo_dev.hpp xor3; the padded range window instead of a `k < K` select per element in echo_range_sl_kernel;
beamsum_coef_kernel in front of the fused route), against in-tree code that keeps the earlier form:
  * isac_mono_static_sensing_dev keeps beamsum_kernel + coef_kernel + echo_spectral_kernel: the fused entry point must store the same echo grid BIT FOR BIT (same D, hence
    the same coefficient vectors from the one-launch beam-sum; same Philox field);
  * range_kernel on the stored grid keeps its select: the fused kernel's range rows may differ in the sign of exact zeros only, so the |rdm|^2 window compares equal
    numerically and every antenna's CFAR list is identical;
  * the lazy grid (echo_range_sl_kernel<., 1, false> + cov_lazy_kernel) materialises bit for bit to the array, Ra within the bound of test_gpu_lazy_echo.py (1e-13: same
    terms, another summation order), estimates identical.
Nfft = nIFFT = 4096, 30 kHz, 14 symbols, Philox spectral noise.  K: 288 (no whole 512-row block of the IFFT input), 3072 (ends on a block boundary), 3084 (12 rows into
block 6), 3276 (the bench value); 64 antennas, 49 (the smallest natively lazy count) at K = 3084; one target, two targets with different delays, a delay shift below the
cyclic prefix (86 samples of 288) and one beyond it (390 > 352)."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest

from conftest import load_pkg

pytestmark = pytest.mark.gpu

NEAR, MID, FAR = (100.0, 20.0, 1.5), (-250.0, 80.0, 1.5), (470.0, 60.0, 1.5)      # delay shifts 86, 216, 390 samples (Ts = 1 / 122.88 MHz); CP = 288 / 352 samples


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def _scene(pkg, nrb, n_ants, targets, velocity, seed, n_sym=14):
    """conftest.make_scene's recipe with Nfft = nIFFT = 4096 at every K (nrOFDMInfo would pick Nfft = 512 at 24 PRB)."""
    import oracle as O
    ci = SimpleNamespace(NRBsDL=nrb, SubcarrierSpacing=30)
    wi = SimpleNamespace(Nfft=4096, SampleRate=4096 * 30e3, SymbolsPerSlot=14, SlotsPerSubframe=2)
    cell = O.default_cell_params(n_ants=n_ants, target_pos=targets, velocity=velocity)
    rng = np.random.default_rng(seed)
    k = 12 * nrb
    bits = rng.integers(0, 2, (2, k, n_sym, n_ants)) * 2 - 1
    tx_grid = np.asfortranarray((bits[0] + 1j * bits[1]) / np.sqrt(2.0))
    amp = float(O.db2mag(cell.gNBTxPower - 30)) * np.sqrt(4096 ** 2 / (k * n_ants))
    tx_wave = np.asfortranarray(O.ofdm_modulate(tx_grid, 4096, 30) * amp)
    rp = pkg.sensing.radarParams(cell, ci, wi)
    rp.nIFFT = 4096                                                          # radarParams.m:69 gives 512 at K = 288; the fused kernel is the 4096-point one
    rp.rRes = 299792458.0 / (2 * 30e3 * rp.nIFFT)                            # :71
    return SimpleNamespace(carrier=ci, rp=rp, cf=pkg.sensing.detection.cfar2D(rp), tx_grid=tx_grid, tx_wave=tx_wave, los=np.ones(len(targets), dtype=np.uint8))


def _fft2d(pkg, ctx, rp, cf, grid, d_txg, reuse):
    """(est | None, debug); a scene without a CFAR detection raises NO_DETECTION on every route alike -- window, lists and Ra are still there to compare."""
    from importlib import import_module
    try:
        return pkg.sensing.estimation.fft2D(rp, cf, grid, d_txg, return_debug=True, reuse_range=reuse)
    except pkg.IsacError as e:
        assert e.name == "NO_DETECTION"
        return None, import_module(pkg.__name__ + ".sensing.estimation.fft2D").fft2D_debug(ctx, grid.shape[2])


def _same(a, b, what):
    (est_a, dbg_a), (est_b, dbg_b) = a, b
    pa, pb = np.asarray(dbg_a.power_window), np.asarray(dbg_b.power_window)
    assert pa.shape == pb.shape and bool((pa == pb).all()), what + ": |rdm|^2 window"        # numeric ==: -0.0 equals +0.0
    assert len(dbg_a.detections) == len(dbg_b.detections) and all(np.array_equal(x, y) for x, y in zip(dbg_a.detections, dbg_b.detections)), what + ": CFAR lists"
    assert (est_a is None) == (est_b is None), what
    if est_a is not None:
        assert np.array_equal(est_a.rngEst, est_b.rngEst) and np.array_equal(est_a.velEst, est_b.velEst) and np.array_equal(est_a.aziEst, est_b.aziEst), what + ": estimates"


def _bits(x):
    return np.ascontiguousarray(np.asarray(x).ravel(order="K")).view(np.uint64)


def _check(pkg, sc, d_wave_host, shape, seed):
    ctx = pkg.Context()
    d_wave, d_txg = ctx.to_device(d_wave_host), ctx.to_device(sc.tx_grid)
    kw = dict(nfft=4096, ctx=ctx, seed=seed, noise_domain="spectral")
    # the route this change leaves alone: beamsum_kernel + coef_kernel + echo_spectral_kernel, then range_kernel on the stored grid
    plain = pkg.sensing.monoStaticSensing(d_wave, shape, sc.carrier, sc.rp, sc.los, **kw)
    g_plain = plain.numpy()
    r_plain = _fft2d(pkg, ctx, sc.rp, sc.cf, plain, d_txg, False)
    # fused, array form
    arr = pkg.sensing.monoStaticSensing(d_wave, shape, sc.carrier, sc.rp, sc.los, fuse_fft2d=(sc.rp, sc.cf, d_txg), **kw)
    r_arr = _fft2d(pkg, ctx, sc.rp, sc.cf, arr, d_txg, True)
    g_arr = arr.numpy()
    assert g_arr.shape == g_plain.shape and np.array_equal(_bits(g_arr), _bits(g_plain)), "echo grid: fused entry point vs isac_mono_static_sensing_dev"
    _same(r_plain, r_arr, "fused range rows vs range_kernel")
    assert np.array_equal(r_arr[1].Ra, r_plain[1].Ra)                       # the same array through the same covariance kernel
    # fused, lazy form
    lz = pkg.sensing.monoStaticSensing(d_wave, shape, sc.carrier, sc.rp, sc.los, fuse_fft2d=(sc.rp, sc.cf, d_txg), lazy=True, **kw)
    r_lz = _fft2d(pkg, ctx, sc.rp, sc.cf, lz, d_txg, True)
    _same(r_arr, r_lz, "lazy vs array")
    ra_l, ra_a = np.asarray(r_lz[1].Ra), np.asarray(r_arr[1].Ra)
    assert float(np.abs(ra_l - ra_a).max() / np.abs(ra_a).max()) < 1e-13
    assert np.array_equal(_bits(lz.numpy()), _bits(g_arr)), "materialised lazy grid vs array"
    ctx.close()
    return g_arr


@pytest.mark.parametrize("nrb,n_ants,targets,velocity", [
    (24, 64, (NEAR,), (7.0,)),                       # K = 288
    (256, 64, (NEAR, MID), (10.0, -6.0)),            # K = 3072, two delays
    (257, 49, (FAR,), (-4.0,)),                      # K = 3084, shift beyond the cyclic prefix
    (273, 64, (NEAR, FAR), (7.0, 3.0)),              # K = 3276
])
def test_fused_and_lazy_routes_match_the_plain_route(pkg, nrb, n_ants, targets, velocity):
    sc = _scene(pkg, nrb, n_ants, targets, velocity, seed=100 + nrb)
    g = _check(pkg, sc, sc.tx_wave, sc.tx_grid.shape, seed=0xD1E7 + nrb)
    assert g.shape == (12 * nrb, 14, n_ants) and g.any()


def test_zero_padded_wide_grid(pkg):
    """txDimension(2) beyond the waveform's whole symbols (monoStaticSensing.m:19-21): the 14th column is never synthesised -- zeros in the array, and a zero range column --
    and a transmit-silent column inside the waveform takes the fused kernel's not-`live` early return (its products are signed zeros now, not selected zeros)."""
    sc = _scene(pkg, 257, 64, (NEAR,), (7.0,), seed=77)
    sc.tx_grid[:, 5, :] = 0                                                  # silent column: rx .* conj(0)
    wave = np.asfortranarray(sc.tx_wave[:sc.tx_wave.shape[0] - 3000])        # the last symbol is incomplete: 13 whole symbols, txDimension says 14
    g = _check(pkg, sc, wave, sc.tx_grid.shape, seed=0x51DE)
    assert g.shape[1] == 14 and not g[:, 13, :].any() and g[:, 12, :].any()
