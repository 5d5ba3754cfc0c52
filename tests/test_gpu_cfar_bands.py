"""The CPI's detector and lists at guard / training bands other than the default (2, 2), (1, 1): fft2D on the scenes of tests/_cfar_band_cases.py with tail fusion on
(cfar_panel_kernel + cfar_merge_kernel where tail_fusable() allows) and off (cfar_window_kernel), against the oracle and against each other.  The table puts hr != hc and
gr != gc in both orders through each Doppler kernel and both range transforms, sits on both sides of each limit that picks the detector, and holds a zone that neither detector
takes and one in which nothing detects; tests/test_cfar_band_cases_cpu.py proves all of that, and the 1e-9 decision margin of every scene, from the oracle alone.  So lists,
counts, indices and the comparison between the two contexts are exact here, values are held to the suite's RTOL, and nothing is skipped."""
from __future__ import annotations

import numpy as np
import pytest

import oracle as O
import _cfar_band_cases as T
from conftest import load_pkg
from test_gpu_parity import RTOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def _config(pkg, o, guard, train):
    rp = pkg.sensing.radarParams(o.sc.cell, o.sc.carrier, o.sc.wave)
    rp.Pfa = o.cfg.Pfa
    cf = pkg.sensing.detection.cfar2D(rp)
    cf.cfarDetector2D.GuardBandSize, cf.cfarDetector2D.TrainingBandSize = guard, train
    assert np.array_equal(cf.CUTIdx, o.cfg.CUTIdx)
    return rp, cf


def _both(pkg, case, ctxs, default_bands=False):
    """fft2D of the case's scene on ctxs = (tail fusion on, tail fusion off), everything checked; returns the fused context's (estimates, debug) or the error name."""
    o = T.oracle_of(case, default_bands)
    sc, g = o.sc, o.geom
    guard, train = o.cfg.GuardBandSize, o.cfg.TrainingBandSize
    out, err = [], []
    for c, fused in zip(ctxs, (True, False)):
        c.set_tail_fusion(fused)
        rp, cf = _config(pkg, o, guard, train)
        try:
            out.append(pkg.sensing.estimation.fft2D(rp, cf, c.to_device(o.echo), c.to_device(sc.tx_grid), return_debug=True))
        except pkg.IsacError as e:
            err.append(e.name)
    kind = "detect" if default_bands else case.kind
    if kind != "detect":
        assert not out and err == [dict(quiet="NO_DETECTION", refused="UNSUPPORTED")[kind]] * 2, (out, err)
        return err[0]
    assert not err, err
    (e1, d1), (e0, d0) = out
    # the power window
    p_ref = np.abs(o.dbg.rdm[g.first_row - 1:g.first_row - 1 + g.nr, g.first_col - 1:g.first_col - 1 + g.nc, :]) ** 2
    for d in (d1, d0):
        assert d.power_window.shape == (g.n_cut_rows + 2 * g.hr, g.n_cut_cols + 2 * g.hc, sc.A)
        assert (d.first_row, d.first_col) == (g.row0 - g.hr, g.col0 - g.hc)
    werr = T.rel(d1.power_window, p_ref)
    print(f"{case.name}{' (default bands)' if default_bands else ''}: {T.doppler_kernel_of(g, int(sc.rp.nFFT))} window error {werr:.3e} = {werr / RTOL:.3g} RTOL")
    assert werr < RTOL
    assert np.array_equal(d1.power_window, d0.power_window)
    # the lists
    for a in range(sc.A):
        want = o.dbg.detections[a]
        assert np.array_equal(d1.detections[a], want), f"antenna {a}: panel route vs oracle"
        assert np.array_equal(d0.detections[a], want), f"antenna {a}: window route vs oracle"
        assert np.array_equal(d1.det_pow[a], d0.det_pow[a]), f"antenna {a}"
        r, c = d1.detections[a]
        assert np.array_equal(d1.det_pow[a], d1.power_window[r - d1.first_row, c - d1.first_col, a])
        assert np.all(np.diff(c.astype(np.int64) * 100000 + r) > 0)               # CUT order: column slowest, row fastest
    # the estimates
    for e, d in ((e1, d1), (e0, d0)):
        assert np.array_equal(e.rngEst, o.est.rngEst) and np.array_equal(e.velEst, o.est.velEst) and np.array_equal(e.aziEst, o.est.aziEst)
        assert np.array_equal(d.Ra, d.Ra.conj().T) and T.rel(d.Ra, o.dbg.Ra) < RTOL
    return e1, d1


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_fft2d_at_other_bands(pkg, case):
    ctxs = (pkg.Context(), pkg.Context())
    try:
        got = _both(pkg, case, ctxs)
        if case.kind == "refused":                               # the refusal leaves the contexts usable: the same zone at the default bands
            assert got == "UNSUPPORTED"
            assert case.name in T.DEFAULT_BAND_RERUNS
            _both(pkg, case, ctxs, default_bands=True)
        elif case.kind == "quiet":
            assert got == "NO_DETECTION"
        elif case.pfa == 0.5:
            assert min(x.shape[1] for x in got[1].detections) > 4096
    finally:
        for c in ctxs:
            c.close()


def test_other_bands_repeated_and_reshaped_calls_on_one_context(pkg):
    """Nothing carries over when hr, hc, pr or n_panels change between calls: panel detector (pr = 8), window detector, the default bands, other window dimensions, 256 panels,
    a quiet zone and a refused one in between, each answer checked in full and the repeated ones against the first."""
    ctxs = (pkg.Context(), pkg.Context())
    C = T.CASE
    assert "pr8_panel" in T.DEFAULT_BAND_RERUNS
    first = _both(pkg, C["pr8_panel"], ctxs)
    seq = [("pr6_window", False), ("pr8_panel", True), ("nrb273_g31_t12", False), ("pr8_panel", False), ("panels_256", False), ("nrb24_nfft64_g13_t21", False),
           ("quiet", False), ("pr8_panel", False), ("refused", False), ("hc5_full", False), ("pr6_window", False), ("pr8_panel", False)]
    for name, default_bands in seq:
        got = _both(pkg, C[name], ctxs, default_bands)
        if name == "pr8_panel" and not default_bands:
            assert np.array_equal(got[0].rngEst, first[0].rngEst) and np.array_equal(got[1].power_window, first[1].power_window)
            assert all(np.array_equal(x, y) for x, y in zip(got[1].det_pow, first[1].det_pow))
    for c in ctxs:
        c.close()


def _same(d_a, d_b, e_a, e_b):
    assert np.array_equal(d_a.power_window, d_b.power_window) and (d_a.first_row, d_a.first_col) == (d_b.first_row, d_b.first_col)
    assert all(np.array_equal(x, y) for x, y in zip(d_a.detections, d_b.detections)) and all(np.array_equal(x, y) for x, y in zip(d_a.det_pow, d_b.det_pow))
    assert np.array_equal(e_a.rngEst, e_b.rngEst) and np.array_equal(e_a.velEst, e_b.velEst) and np.array_equal(e_a.aziEst, e_b.aziEst)


def _against(o, est, dbg):
    g = o.geom
    assert dbg.power_window.shape == (g.nr, g.nc, o.sc.A) and (dbg.first_row, dbg.first_col) == (g.first_row, g.first_col)
    assert T.rel(dbg.power_window, np.abs(o.dbg.rdm[g.first_row - 1:g.first_row - 1 + g.nr, g.first_col - 1:g.first_col - 1 + g.nc, :]) ** 2) < RTOL
    for a in range(o.sc.A):
        assert np.array_equal(dbg.detections[a], o.dbg.detections[a]), f"antenna {a}"
    assert np.array_equal(est.rngEst, o.est.rngEst) and np.array_equal(est.velEst, o.est.velEst) and np.array_equal(est.aziEst, o.est.aziEst)


def test_cached_and_fused_range_routes_share_the_row_window(pkg):
    """CutRows = CUT rows +- hr: at hr = 12 != hc = 2 the window's rows lie in two 512-row blocks of the range transform where the CUT rows alone lie in one (asserted in
    tests/test_cfar_band_cases_cpu.py), so a route that sized its row window by anything but hr would form the wrong blocks.  The equalities of
    test_gpu_parity.test_fused_range_stage_is_identical and of the last block of test_fft2d_range_window_position, each form against the oracle as well."""
    case = T.RANGE_WINDOW_CASE
    o = T.oracle_of(case)
    sc = o.sc
    ctx = pkg.Context()
    try:
        rp, cf = _config(pkg, o, case.guard, case.train)
        fft2D, sense = pkg.sensing.estimation.fft2D, pkg.sensing.monoStaticSensing
        d_wave, d_noise, d_txg = ctx.to_device(sc.tx_wave), ctx.to_device(sc.noise), ctx.to_device(sc.tx_grid)
        # the scene's time-domain noise: unfused, then fused + cached range rows
        e0 = sense(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=d_noise, nfft=4096, ctx=ctx)
        assert T.rel(e0.numpy(), o.echo) < RTOL
        est0, dbg0 = fft2D(rp, cf, e0, d_txg, return_debug=True)
        e1 = sense(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=d_noise, nfft=4096, fuse_fft2d=(rp, cf, d_txg), ctx=ctx)
        est1, dbg1 = fft2D(rp, cf, e1, d_txg, return_debug=True, reuse_range=True)
        assert np.array_equal(e0.numpy(), e1.numpy())
        _same(dbg0, dbg1, est0, est1)
        _against(o, est0, dbg0)
        # seeded spectral noise: plain; fused + cached range rows; the fused call's grid through a plain fft2D (which never trusts the cache)
        kw = dict(nfft=4096, seed=T.SPECTRAL_SEED, noise_domain="spectral", ctx=ctx)
        ea = sense(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, **kw)
        est_a, dbg_a = fft2D(rp, cf, ea, d_txg, return_debug=True)
        eb = sense(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, fuse_fft2d=(rp, cf, d_txg), **kw)
        est_b, dbg_b = fft2D(rp, cf, eb, d_txg, return_debug=True, reuse_range=True)
        ec = sense(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, fuse_fft2d=(rp, cf, d_txg), **kw)
        est_c, dbg_c = fft2D(rp, cf, ec, d_txg, return_debug=True)
        grid = ea.numpy()
        assert np.array_equal(eb.numpy(), ec.numpy())
        _same(dbg_a, dbg_b, est_a, est_b)
        _same(dbg_a, dbg_c, est_a, est_c)
        # ... and the oracle on that grid; the restated field (CPU test) says the device's grid is decidable, its own margin is asserted all the same
        ref = T.spectral_reference_of(case)
        eta = float(np.sqrt(sc.rp.N0 / 2.0) * np.sqrt(sc.wave.Nfft)) * O.philox.SPECTRAL_NOISE_ATOL + RTOL * float(np.abs(ref.echo).max())   # test_gpu_spectral.py's bound
        assert float(np.abs(grid - ref.echo).max()) <= eta, "not the restated Philox field"
        og = T.chain_on(sc, o.cfg, np.asfortranarray(grid))
        print(f"{case.name}: margins on the device's grid {['%.2e' % m for m in og.margin]}")
        assert min(og.margin) > 1e-9, "scene too close to a threshold"
        for est, dbg in ((est_a, dbg_a), (est_b, dbg_b), (est_c, dbg_c)):
            _against(og, est, dbg)
    finally:
        ctx.close()
