"""The LAZY CPI -- the path bench.py times: isac_mono_static_sensing_fused_dev with d_echo_grid == NULL on the spectral Philox route, 49..64 antennas, one or two LoS targets:
echo_range_sl_kernel<Q, 1, false>, cov_lazy_kernel<Q>, the one-launch beam-sum -- against the ORACLE, not against the library's array form (every other lazy test compares the
two forms of one library: what they share -- spectral_echo_value, the Philox / Box-Muller pieces, the coefficient vectors, the steering table -- and what only the lazy form has
-- the per-antenna counter arithmetic, pair rows (k, k + 512), the masked partner half of a partial block pair, the `ga + 32 >= A` mask, 1 / (K L_out), the compaction of LoS
targets around a blocked one -- can be wrong on both sides of those comparisons).  One lazy call per case, the grid materialised, two comparisons:

  (A) same field, independent arithmetic: the materialised grid through O.fft2d (rdm_explicit): |rdm|^2 window <= 1e-10 (test_gpu_fullsize.RTOL), every antenna's CFAR list,
      rngEst / velEst / aziEst identical, Ra <= 1e-10 and exactly Hermitian; NO_DETECTION on both sides where no CUT fires.  Two guards from the oracle's numbers alone say
      whether the input can be compared exactly: no CUT cell within 1e-7 (relative) of its threshold, eigenvalue gap at the signal / noise split > 1e-9 w[0]
      (test_gpu_music_subspace.py's degenerate-cluster rule).  A case that trips one FAILS as an unsuitable input; tests/test_lazy_cpi_reference_cpu.py holds every case a
      decade inside both on the reference grid.
  (B) independent field: the grid against tests/_lazy_cpi_reference.py's (the oracle's time-domain chain fed the restated Philox field; nothing from the device), element by
      element:   |g - E| <= eta := sig SPECTRAL_NOISE_ATOL + 1e-10 max|E|   (test_gpu_spectral.py: float32 hardware Box-Muller against its float32 restatement), and
                 |Ra - Ra_ref|[a, b] <= eta (m_a + m_b) + eta^2 + 1e-12 max|Ra_ref|,   m_a = mean_n |E[n, a]|
      (an element error <= eta on a product of two elements; the summation-order allowance of test_covariance_mfma) -- every term from the reference.  This is what a wrong
      counter, antenna stride or normalisation fails, which (A) passes when the materialiser shares it.

Shapes: tests/_lazy_cpi_reference.TABLE (what each reaches: tests/test_lazy_cpi_reference_cpu.py), the antenna counts 48 and 65 on either side of the native route (the grid in
a context-owned buffer: the same two comparisons), and six seeded scenes through (A).  Observed maxima go to record_property."""
from __future__ import annotations

from importlib import import_module

import numpy as np
import pytest

import _lazy_cpi_reference as R
from conftest import load_pkg

pytestmark = pytest.mark.gpu
RTOL = R.RTOL


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def _lazy_cpi(pkg, sc):
    """One lazy call + cached fft2D -> (est | None, debug, materialised grid)."""
    ctx = pkg.Context()
    try:
        cf = pkg.sensing.detection.cfar2D(sc.rp)
        assert (cf.cfarDetector2D.GuardBandSize, cf.cfarDetector2D.TrainingBandSize) == R.DEFAULT_BANDS
        cf.cfarDetector2D.GuardBandSize, cf.cfarDetector2D.TrainingBandSize = sc.case.bands
        d_wave, d_txg = ctx.to_device(sc.tx_wave), ctx.to_device(sc.tx_grid)
        lz = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, sc.rp, sc.los, nfft=4096, ctx=ctx, lazy=True, fuse_fft2d=(sc.rp, cf, d_txg),
                                           seed=sc.case.noise_seed, noise_domain="spectral")
        assert lz.shape == sc.tx_grid.shape
        try:
            est, dbg = pkg.sensing.estimation.fft2D(sc.rp, cf, lz, d_txg, return_debug=True, reuse_range=True)
        except pkg.IsacError as e:
            assert e.name == "NO_DETECTION"
            est, dbg = None, import_module(pkg.__name__ + ".sensing.estimation.fft2D").fft2D_debug(ctx, sc.A)
        return est, dbg, lz.numpy()
    finally:
        ctx.close()


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(float(np.abs(np.asarray(b)).max()), 1e-300))


def _compare_same_field(sc, est, dbg, g, record_property):
    """(A): the oracle's fft2D on the grid the device materialised."""
    o = R.oracle_chain(sc, g)
    record_property("cfar_margin", o.cfar_margin)
    record_property("eig_gap_over_w0", o.eig_gap)
    record_property("detections", o.n_det)
    print(f"{sc.case.name}: oracle detections {o.n_det}, CFAR margin {o.cfar_margin:.3e}, eigenvalue gap {o.eig_gap:.3e} w[0]")
    assert o.cfar_margin > 1e-7, f"unsuitable input: a CUT cell lies within {o.cfar_margin:.2e} of its threshold -- no exact comparison of the CFAR lists is meaningful"
    assert o.eig_gap > 1e-9, f"unsuitable input: eigenvalue gap {o.eig_gap:.2e} w[0] at the signal / noise split -- the MUSIC peaks are undefined"
    r0, c0 = dbg.first_row, dbg.first_col
    nr, nc, na = dbg.power_window.shape
    assert na == sc.A
    hr, hc = (o.cfg.GuardBandSize[i] + o.cfg.TrainingBandSize[i] for i in range(2))
    assert (r0, c0) == (o.cfg.rowRange[0] - hr, o.cfg.colRange[0] - hc) and (nr, nc) == (o.cfg.rowRange[1] - o.cfg.rowRange[0] + 1 + 2 * hr, o.cfg.colRange[1] - o.cfg.colRange[0] + 1 + 2 * hc)
    w_err = _rel(dbg.power_window, np.abs(o.rdm[r0 - 1:r0 - 1 + nr, c0 - 1:c0 - 1 + nc, :]) ** 2)
    ra_err = _rel(dbg.Ra, o.Ra)
    record_property("window_err_over_rtol", w_err / RTOL)
    record_property("ra_err_over_rtol", ra_err / RTOL)
    print(f"{sc.case.name}: |rdm|^2 window {w_err:.3e}, Ra {ra_err:.3e} (bound {RTOL:g})")
    assert w_err < RTOL
    assert len(dbg.detections) == sc.A
    for a in range(sc.A):
        assert np.array_equal(dbg.detections[a], o.detections[a]), f"antenna {a}"
    assert (est is None) == (o.est is None), "NO_DETECTION on one side only"
    if est is not None:
        assert np.array_equal(est.rngEst, o.est.rngEst) and np.array_equal(est.velEst, o.est.velEst) and np.array_equal(est.aziEst, o.est.aziEst), (est, o.est)
    assert ra_err <= RTOL and np.array_equal(dbg.Ra, dbg.Ra.conj().T)
    return o


def _compare_independent_field(sc, dbg, g, e, ra_ref, m, eta, record_property):
    """(B): grid and Ra against the reference's, every bound from the reference."""
    assert g.shape == e.shape
    e_err = float(np.abs(g - e).max())
    bound = R.covariance_bound(eta, m, ra_ref)
    r_err = float((np.abs(dbg.Ra - ra_ref) / bound).max())
    record_property("echo_err_over_eta", e_err / eta)
    record_property("ra_err_over_bound", r_err)
    print(f"{sc.case.name}: |g - E| {e_err:.3e} = {e_err / eta:.3f} eta; Ra error {r_err:.3f} of its bound; eta / max|E| {eta / float(np.abs(e).max()):.2e}")
    assert e_err <= eta
    assert not g[:, sc.L_whole:, :].any()                                  # monoStaticSensing.m:19-21: the padding columns are zeros
    assert r_err <= 1.0


@pytest.mark.parametrize("case", tuple(R.TABLE) + tuple(R.NEIGHBOURS), ids=lambda c: c.name)
def test_lazy_cpi_against_the_oracle(pkg, case, record_property):
    sc, e, ra_ref, m, eta = R.reference_of(case, pkg.sensing.radarParams)
    est, dbg, g = _lazy_cpi(pkg, sc)
    _compare_independent_field(sc, dbg, g, e, ra_ref, m, eta, record_property)
    _compare_same_field(sc, est, dbg, g, record_property)


def test_lazy_cpi_at_asymmetric_bands(pkg, record_property):
    """GuardBandSize (10, 1), TrainingBandSize (6, 3): the lazy range kernel's row window (CUT rows +- 16) and the Doppler kernel's columns (+- 4) at half sizes that differ
    from each other and from the default 3; both comparisons, at the bounds every other case is held to."""
    case = R.BAND_CASE
    sc, e, ra_ref, m, eta = R.reference_of(case, pkg.sensing.radarParams)
    est, dbg, g = _lazy_cpi(pkg, sc)
    _compare_independent_field(sc, dbg, g, e, ra_ref, m, eta, record_property)
    o = _compare_same_field(sc, est, dbg, g, record_property)
    assert dbg.power_window.shape[:2] == (o.cfg.rowRange[1] - o.cfg.rowRange[0] + 1 + 32, o.cfg.colRange[1] - o.cfg.colRange[0] + 1 + 8)
    assert o.n_det > sc.A and est is not None


@pytest.mark.parametrize("seed", R.SWEEP_SEEDS)
def test_lazy_cpi_seeded_sweep(pkg, seed, record_property):
    """Comparison (A) on seeded scenes: nrb from {24, 43, 86, 129, 273}, 49..64 antennas, one or two targets anywhere in the detection area, random LoS flags."""
    sc = R.build_scene(R.sweep_case(seed), pkg.sensing.radarParams)
    est, dbg, g = _lazy_cpi(pkg, sc)
    _compare_same_field(sc, est, dbg, g, record_property)
