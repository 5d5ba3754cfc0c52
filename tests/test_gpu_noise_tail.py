"""The split covariance's noise term in two kernels (csrc/noise_walk.hpp): cov_noise_beam_kernel walks the full slabs of the lazy grid alone, cov_noise_tail_kernel forms the
half slabs -- the rows whose partner k + 512 lies beyond K -- two to a slab, on the context's second stream, and appends its partials.  The scenes and helpers are those of
tests/test_gpu_lazy_split.py; nIFFT 4096 at 30 kHz, 14 symbols, 49 and 64 antennas, one and two LoS targets.

  shapes   PRBs  K     what the packing does there
           24    288   only half slabs, an even count (36 -> 18 packed); the main kernel walks no slab at all and sums every beam unit in the loop behind the slabs
           25    300   only half slabs, the last one partial (rows 296..299), an odd count (37 -> 19 packed, the last with an empty second half)
           52    624   full (14) and half (50) slabs inside one 1024-block
           106   1272  31 half slabs in the second block: one packed slab with an empty second half
           273   3276  the bench's K: 192 full slabs, 26 half slabs -> 13 packed
  asserted on the split route: Ra <= 1e-13 of the array form AND of the regenerating route (the project's bound for another summation order; the packed walk is a third
           order) and exactly Hermitian; the |rdm|^2 window (the range rows), every antenna's CFAR list and every estimate byte-identical to the regenerating route and to
           the array form; isac_ctx_get_lazy_cov_route_used reports the split route (asserted inside the shared helper for every lazy run).
  beam-sums  cov_noise_beam_kernel addresses the waveform through ONE descriptor, the antenna in the load's scalar offset; a padding antenna slot (5, 4 and 2 of them in a
           unit's last step at 49, 50 and 64 antennas) must still read a true zero.  The waveform handed to the calls is the first A columns of a device array of 72, whose
           columns from A on -- the samples behind every padding slot -- hold NaN: one of them reaching a beam-sum makes it NaN whatever the steering image holds.  The
           beam-sums themselves are not exported; the coefficient vectors are their products with the phase ramps and the grid is D a + sig w, so the materialised lazy grid
           bit-equal to the array the non-lazy call stores (beamsum_kernel / beamsum_coef_kernel) is the beam-sums inside the demodulation windows bit for bit.  273 PRB x 28
           symbols: the smallest shape of the suite at which a workgroup's slab steps outlast a beam unit, i.e. the loads beside the slabs are the ones that run."""
from __future__ import annotations

from importlib import import_module

import numpy as np
import pytest

from conftest import load_pkg
from test_gpu_lazy_split import _cpi, _fft2d, _same_lists, _scene, rel

pytestmark = pytest.mark.gpu

SPLIT, REGENERATE = 0, 1


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.mark.parametrize("q", [1, 2])
@pytest.mark.parametrize("n_ants", [49, 64])
@pytest.mark.parametrize("nrb", [24, 25, 52, 106, 273])
def test_packed_half_slabs_match_the_regenerating_route_and_the_array_form(pkg, nrb, n_ants, q, record_property):
    sc = _scene(pkg, nrb, 14, n_ants, q)
    seed = sc.case.noise_seed
    est_a, dbg_a, g_a = _cpi(pkg, sc, seed, None)
    est_0, dbg_0, g_0 = _cpi(pkg, sc, seed, SPLIT)              # (asserts that the covariance took the split route)
    est_1, dbg_1, g_1 = _cpi(pkg, sc, seed, REGENERATE)
    e_arr, e_reg = rel(dbg_0.Ra, dbg_a.Ra), rel(dbg_0.Ra, dbg_1.Ra)
    record_property("ra_split_vs_array", e_arr)
    record_property("ra_split_vs_regenerating", e_reg)
    print(f"K {12 * nrb} A {n_ants} Q {q}: Ra of the split route against the array form {e_arr:.3e}, against the regenerating route {e_reg:.3e}")
    assert e_arr <= 1e-13 and e_reg <= 1e-13
    assert np.array_equal(dbg_0.Ra, dbg_0.Ra.conj().T)
    assert np.array_equal(g_0, g_1) and np.array_equal(g_0, g_a)
    _same_lists((est_0, dbg_0), (est_1, dbg_1))                # the range rows (power window), every CFAR list, every estimate
    _same_lists((est_0, dbg_0), (est_a, dbg_a))


def _grid_behind_nan_columns(pkg, sc, route):
    """The materialised echo grid of the scene, its waveform handed over as the first A columns of a [T x 72] device array whose other columns are NaN."""
    dev_array = import_module(pkg.__name__ + "._lib").DeviceArray
    ctx = pkg.Context()
    try:
        if route is not None:
            ctx.set_lazy_cov_route(route)
        t, a = sc.tx_wave.shape
        wide = np.full((t, 72), complex(np.nan, np.nan), dtype=np.complex128, order="F")
        wide[:, :a] = sc.tx_wave
        d_wide = ctx.to_device(wide)
        d_wave = dev_array(ctx, d_wide.ptr, (t, a), np.complex128, owner=False)      # column-major: the first A columns are the waveform
        d_txg = ctx.to_device(sc.tx_grid)
        cf = pkg.sensing.detection.cfar2D(sc.rp)
        g = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, sc.rp, sc.los, nfft=4096, fuse_fft2d=(sc.rp, cf, d_txg), ctx=ctx, lazy=route is not None,
                                          seed=sc.case.noise_seed, noise_domain="spectral")
        _, dbg = _fft2d(pkg, sc.rp, cf, g, d_txg, ctx)
        if route is not None:
            assert ctx.lazy_cov_route_used() == route
        return g.numpy(), dbg
    finally:
        ctx.close()


@pytest.mark.parametrize("q", [1, 2])
@pytest.mark.parametrize("n_ants", [49, 50, 64])
def test_beam_sums_keep_beamsum_kernels_bits_with_nan_behind_the_padding_slots(pkg, n_ants, q):
    sc = _scene(pkg, 273, 28, n_ants, q)
    g_arr, dbg_arr = _grid_behind_nan_columns(pkg, sc, None)
    g_split, dbg_split = _grid_behind_nan_columns(pkg, sc, SPLIT)
    assert np.isfinite(g_split).all() and np.isfinite(dbg_split.Ra).all()
    assert np.array_equal(g_split, g_arr)
    assert np.array_equal(dbg_split.power_window, dbg_arr.power_window)
