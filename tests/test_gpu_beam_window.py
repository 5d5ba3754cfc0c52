"""The window-walking beam-sum (beamsum_coef_kernel over the units of csrc/beam_window.hpp, steering vectors in its argument block) against the route that keeps
beamsum_kernel + coef_kernel over all of [0, T) with an uploaded steering table: isac_mono_static_sensing_dev.  That route is the reference; the fused entry point
(monoStaticSensing(fuse_fft2d=...)) with a caller-owned echo grid must store the same grid BIT FOR BIT -- same D, hence the same coefficient vectors inside every
demodulation window, zeros in front of a target's delay included, and the same steering table written by the kernel itself.

The new kernel sits in front of the fused spectral route only (Nfft = nIFFT = 4096, a spectral noise mode, one or two LoS targets), so those are the cases that reach it:
A = 2 ... 4, 1 ... 29 symbols, a waveform 37 samples longer than its symbols (no multiple of 256), target delays d of {0, 1, cp/2 - 1, cp/2, cp/2 + 1, cp, cp + 1, 2 cp}
(cp = 288), two targets with equal and unequal delays, one pair with d_max - d_min > cp (the ranges of neighbouring symbols would overlap: one walk over every sample),
noise injected as zeros or drawn by Philox on both routes alike.  One natively lazy case (49 antennas, K = 288) compares isac_echo_grid_materialize_dev the same way.
At Nfft = 128 and 256 (noise off, and zeros injected) the fused entry point has no fused kernel and runs the reference route itself: those cases pin the contract there."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import load_pkg

pytestmark = pytest.mark.gpu

CP = {128: 9, 256: 18, 4096: 288}                       # normal cyclic prefix, samples
LIGHTSPEED = 299792458.0


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def _delays(cp):
    return [0, 1, cp // 2 - 1, cp // 2, cp // 2 + 1, cp, cp + 1, 2 * cp]


def _bits(x):
    return np.ascontiguousarray(np.asarray(x).ravel(order="K")).view(np.uint64)


def _scene(pkg, ctx, nfft, nrb, n_ants, n_sym, delays, seed):
    """A random [T x A] transmit waveform (the beam-sum does not care what it carries), T = n_sym whole symbols + 37 samples, a QPSK transmit grid for the range stage, and
    radar parameters whose targets sit at the given delays exactly: range = (d - 1/2) c Ts / 2, so ceil(pathDelay / Ts) = d (basicRadarChannel.m:21-22)."""
    import oracle as O
    ci = SimpleNamespace(NRBsDL=nrb, SubcarrierSpacing=30)
    wi = SimpleNamespace(Nfft=nfft, SampleRate=nfft * 30e3, SymbolsPerSlot=14, SlotsPerSubframe=2)
    q = len(delays)
    cell = O.default_cell_params(n_ants=n_ants, target_pos=tuple((100.0 + 40.0 * i, 20.0 - 30.0 * i, 1.5) for i in range(q)), velocity=tuple(7.0 - 10.0 * i for i in range(q)))
    rp = pkg.sensing.radarParams(cell, ci, wi)
    if nfft == 4096:
        rp.nIFFT = 4096                                                      # the fused kernel is the 4096-point one
        rp.rRes = LIGHTSPEED / (2 * 30e3 * rp.nIFFT)
    rp.range = np.array([max(d - 0.5, 0.0) * LIGHTSPEED / (2.0 * rp.fs) for d in delays])
    car = pkg._lib.Carrier(12 * nrb, nfft, 30, 0)
    t = C.c_int64(0)
    assert ctx.lib.isac_ofdm_waveform_length(C.byref(car), C.c_int32(n_sym), C.byref(t)) == 0
    T = int(t.value) + 37
    rng = np.random.default_rng(seed)
    wave = np.asfortranarray(rng.standard_normal((T, n_ants)) + 1j * rng.standard_normal((T, n_ants)))
    bits = rng.integers(0, 2, (2, 12 * nrb, n_sym, n_ants)) * 2 - 1
    tx_grid = np.asfortranarray((bits[0] + 1j * bits[1]) / np.sqrt(2.0))
    return SimpleNamespace(carrier=ci, rp=rp, cf=pkg.sensing.detection.cfar2D(rp), los=np.ones(q, dtype=np.uint8), shape=tx_grid.shape,
                           d_wave=ctx.to_device(wave), d_txg=ctx.to_device(tx_grid))


def _both_routes(pkg, ctx, sc, nfft, **noise):
    ref = pkg.sensing.monoStaticSensing(sc.d_wave, sc.shape, sc.carrier, sc.rp, sc.los, nfft=nfft, ctx=ctx, **noise).numpy()
    got = pkg.sensing.monoStaticSensing(sc.d_wave, sc.shape, sc.carrier, sc.rp, sc.los, nfft=nfft, ctx=ctx, fuse_fft2d=(sc.rp, sc.cf, sc.d_txg), **noise).numpy()
    assert got.shape == ref.shape == sc.shape and ref.any()
    assert np.array_equal(_bits(got), _bits(ref)), "echo grid: fused entry point vs isac_mono_static_sensing_dev"
    return ref


_D = _delays(288)
CASES_4096 = [(2 + i % 3, (1, 2, 14, 15, 29)[i % 5], (d,)) for i, d in enumerate(_D)] + [
    (3, 15, (144, 144)),                                 # two targets, one delay
    (4, 2, (0, 288)),                                    # d_max - d_min = cp: the ranges of neighbouring symbols touch
    (2, 29, (143, 289)),
    (3, 14, (1, 576)),                                   # d_max - d_min > cp
    (4, 1, (576, 145)),
]


@pytest.mark.parametrize("n_ants,n_sym,delays", CASES_4096)
def test_window_walk_matches_the_full_walk(pkg, n_ants, n_sym, delays):
    ctx = pkg.Context()
    sc = _scene(pkg, ctx, 4096, 24, n_ants, n_sym, delays, seed=1000 * n_sym + sum(delays))
    zeros = ctx.to_device(np.zeros(sc.shape, dtype=np.complex128, order="F"))
    g0 = _both_routes(pkg, ctx, sc, 4096, spectral_noise=zeros)
    g1 = _both_routes(pkg, ctx, sc, 4096, seed=0xBEA0 + n_sym, noise_domain="spectral")
    assert not np.array_equal(g0, g1)
    ctx.close()


@pytest.mark.parametrize("delays", [(144,), (86, 390)])
def test_lazy_native_grid_materialises_to_the_full_walk(pkg, delays):
    """49 antennas (the smallest natively lazy count), K = 288, Philox spectral noise: nothing is stored by the fused call; the materialised grid is the reference route's."""
    ctx = pkg.Context()
    sc = _scene(pkg, ctx, 4096, 24, 49, 14, delays, seed=49 + len(delays))
    kw = dict(nfft=4096, ctx=ctx, seed=0x1A2B, noise_domain="spectral")
    ref = pkg.sensing.monoStaticSensing(sc.d_wave, sc.shape, sc.carrier, sc.rp, sc.los, **kw).numpy()
    lz = pkg.sensing.monoStaticSensing(sc.d_wave, sc.shape, sc.carrier, sc.rp, sc.los, fuse_fft2d=(sc.rp, sc.cf, sc.d_txg), lazy=True, **kw)
    got = lz.numpy()
    assert got.shape == ref.shape and ref.any() and np.array_equal(_bits(got), _bits(ref)), "materialised lazy grid vs isac_mono_static_sensing_dev"
    ctx.close()


@pytest.mark.parametrize("nfft,nrb", [(128, 8), (256, 16)])
def test_small_carriers_keep_the_reference_route(pkg, nfft, nrb):
    ctx = pkg.Context()
    ds = _delays(CP[nfft])
    cases = [(2, 29, (d,)) for d in ds[:4]] + [(4, 15, (d,)) for d in ds[4:]] + [(3, 14, (ds[3], ds[3])), (3, 2, (ds[1], ds[7])), (2, 1, (ds[6], ds[2]))]
    for n_ants, n_sym, delays in cases:
        sc = _scene(pkg, ctx, nfft, nrb, n_ants, n_sym, delays, seed=nfft + n_sym + sum(delays))
        _both_routes(pkg, ctx, sc, nfft)                                                                   # noise off
        _both_routes(pkg, ctx, sc, nfft, spectral_noise=ctx.to_device(np.zeros(sc.shape, dtype=np.complex128, order="F")))
    ctx.close()
