"""The context's cached device tables live in one map keyed by kind and parameters (csrc/isac_common.hpp: TableKey) and are freed with the context.
Two things can go wrong there and nowhere else: two tables that land on one key, and a context torn down while its tables are populated.
  * one context through several numerologies and scan grids gives, bit for bit, what a fresh context gives for each of them, and the oracle's estimates;
  * the UPA scan tables are picked by grid;
  * a context closed with populated tables leaves the next context's results unchanged, and close() twice is harmless.
The sensing calls take host arrays, so the host-pointer entry points (temporary device buffers) are on the path too."""
from __future__ import annotations

import copy

import numpy as np
import pytest

import oracle as O
from conftest import load_pkg, make_scene
from test_gpu_upa_doa import _covariance, _rp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def cases():
    """(scene, azimuth granularity, oracle estimates) of the three configurations: K / nIFFT / nFFT = 288 / 512 / 64 (X) and 612 / 1024 / 128 (Y)."""
    x = make_scene(n_ants=4, n_slots=4, nrb=24, targets=((150.0, 40.0, 1.5),), velocity=(0.0,), num_slots_param=6, zero_s_slots=False)
    y = make_scene(n_ants=6, n_slots=8, nrb=51, targets=((120.0, 60.0, 1.5), (-250.0, 80.0, 1.5)), velocity=(10.0, -6.0), num_slots_param=12, seed=5)
    out = {}
    for name, sc, gran in (("X", x, 1), ("Y", y, 1), ("X/0.5", x, 0.5)):
        rx = O.mono_static_sensing(sc.tx_wave, sc.tx_grid.shape, sc.carrier, sc.rp, sc.los, sc.noise, nfft=sc.wave.Nfft)
        rp = copy.copy(sc.rp)
        rp.azimuthScanGranularity = gran
        out[name] = (sc, gran, O.fft2d(rp, O.cfar2d_config(rp), rx, sc.tx_grid))
    # the scenes exercise something: the oracle detects in all of them
    assert (out["X"][2].rngEst.size, out["X"][2].velEst.size, out["Y"][2].rngEst.size, out["Y"][2].velEst.size) == (3, 1, 6, 4)
    assert np.array_equal(out["X"][2].aziEst, [-97, -83, 90]) and np.array_equal(out["X/0.5"][2].aziEst, [-97.5, -82.5, 90])
    return out


def _run(pkg, ctx, sc, gran):
    rp = pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)
    rp.azimuthScanGranularity = gran
    cf = pkg.sensing.detection.cfar2D(rp)
    echo = pkg.sensing.monoStaticSensing(sc.tx_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=ctx)
    return pkg.sensing.estimation.fft2D(rp, cf, echo, sc.tx_grid, ctx=ctx, return_debug=True)


def _same(e, want):                      # as tests/test_gpu_schedule.py::_same
    return np.array_equal(e.rngEst, want.rngEst) and np.array_equal(e.velEst, want.velEst) and np.array_equal(e.aziEst, want.aziEst)


def _bitwise(got, ref, n_ants):
    (e0, d0), (e1, d1) = got, ref
    assert np.array_equal(d0.power_window, d1.power_window) and np.array_equal(d0.Ra, d1.Ra) and np.array_equal(d0.spectrum_db, d1.spectrum_db)
    for a in range(n_ants):
        assert np.array_equal(d0.detections[a], d1.detections[a]), f"antenna {a}"
    assert _same(e0, e1)


def test_one_context_many_tables(pkg, cases):
    fresh = {}
    for name, (sc, gran, _) in cases.items():
        c = pkg.Context()
        fresh[name] = _run(pkg, c, sc, gran)
        c.close()
    shared = pkg.Context()
    for name in ("X", "Y", "X/0.5", "X"):
        sc, gran, want = cases[name]
        got = _run(pkg, shared, sc, gran)
        _bitwise(got, fresh[name], sc.A)
        assert _same(got[0], want), name
    shared.close()


def test_upa_tables_by_grid(pkg):
    doa = pkg.sensing.estimation.doaEstimation
    ra = _covariance(4, 4, 2, seed=7)

    def scan(ctx, gran):
        rp = _rp(4, 4)
        rp.azimuthScanGranularity = rp.elevationScanGranularity = gran
        doa.music(2, rp, ra, ctx=ctx)
        return ctx.angular_spectrum2d()

    fresh = {}
    for gran in (1, 2):
        c = pkg.Context()
        c.set_upa_doa(True)
        fresh[gran] = scan(c, gran)
        c.close()
    shared = pkg.Context()
    shared.set_upa_doa(True)
    for gran, shape in ((1, (181, 361)), (2, (90, 180)), (1, (181, 361))):
        got = scan(shared, gran)
        assert got.shape == shape
        assert np.array_equal(got, fresh[gran])
    shared.close()


def test_close_with_populated_tables(pkg, cases):
    sc, gran, _ = cases["X"]
    first = pkg.Context()
    ref = _run(pkg, first, sc, gran)
    first.close()
    second = pkg.Context()
    _bitwise(_run(pkg, second, sc, gran), ref, sc.A)
    second.close()
    second.close()                       # harmless
