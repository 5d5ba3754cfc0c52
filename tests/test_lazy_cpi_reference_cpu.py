"""tests/_lazy_cpi_reference.py checked without a GPU: the scene builder's two parameter sets, the reference echo grid and covariance against the oracle's own functions, the
shape table against the slab / mask cases it is there to reach (csrc/cov.hip's arithmetic restated), and -- for every table case, both antenna-count neighbours and every
sweep seed -- the two input-suitability guards of tests/test_gpu_lazy_oracle.py on the REFERENCE grid with a decade to spare: the device's field differs from the reference's by
at most eta per element (a few 1e-9 .. 1e-7 of the grid's maximum), so the spare decade is what keeps the guards valid on the GPU.

What had to be chosen for a scene to have a detection at all (the 4096-point range transform is what the native lazy route requires):
  * numSlots = 2 per slot of the CPI (nFFT = 32 / 64): with the default 20 the 14 live symbols sit in a 256-point Doppler transform whose main lobe covers the CFAR ring;
  * K <= 516 (table cases 1, 2, the two neighbours): the range main lobe is > 16 bins wide, the ring (3 bins out) sits on it, CA-CFAR cannot fire at any Pfa that keeps the
    noise cells quiet -- these cases compare window, empty lists, Ra and NO_DETECTION;
  * K = 1020 / 1032: Pfa = 1e-5 (the cell's parameter, radar.m:15, on both sides): at 1e-9 the threshold is 1.9 x the peak for the same reason;
  * K = 3276: three adjacent range rows fire per target, so the signal / noise split lies inside the noise cluster and its gap is ~ 1e-3 sigma^2: with RCS = 1 the first
    eigenvalue is 1e9 x that (gap 5e-10 w[0]); RCS = 1e-2 on table case 7 and in the sweep brings it to 5e-8 and more."""
from __future__ import annotations

import numpy as np
import pytest

import oracle as O
import _lazy_cpi_reference as R
from conftest import load_pkg

ALL_CASES = tuple(R.TABLE) + tuple(R.NEIGHBOURS) + tuple(R.sweep_case(s) for s in R.SWEEP_SEEDS) + (R.BAND_CASE,)
_chain = {}


def _oracle_on_reference(case):
    if case.name not in _chain:
        sc, e, _, _, _ = R.reference_of(case)
        _chain[case.name] = R.oracle_chain(sc, e)
    return _chain[case.name]


def test_shape_table_is_the_specified_one():
    got = [(c.nrb, c.n_ants, c.los, R.slab_plan(c).L_whole, c.n_sym) for c in R.TABLE]
    assert got == [(24, 64, (1,), 14, 14), (43, 49, (1,), 14, 14), (85, 63, (1, 1), 14, 14), (86, 64, (1,), 13, 14), (86, 56, (1, 1), 27, 28),
                   (129, 64, (1, 0, 1), 14, 14), (273, 64, (0, 1), 14, 14), (273, 50, (1, 1), 28, 28)]
    assert [(c.nrb, c.n_ants, c.los) for c in R.NEIGHBOURS] == [(43, 48, (1,)), (43, 65, (1,))]
    assert R.TABLE[4].silent and R.TABLE[4].zero_from is None and R.TABLE[7].zero_from == 14 and R.TABLE[7].targets == (R.NEAR, R.FAR)
    sweep = [R.sweep_case(s) for s in R.SWEEP_SEEDS]
    assert len(sweep) == 6 and all(c.nrb in R.SWEEP_NRB and 49 <= c.n_ants <= 64 and 1 <= len(c.targets) <= 2 and any(c.los) and c.n_sym == 14 for c in sweep)
    assert {len(c.targets) for c in sweep} == {1, 2} and {c.nrb for c in sweep} == set(R.SWEEP_NRB)


def test_shape_table_reaches_the_slab_and_mask_cases():
    """The slab numbers worked out by hand from csrc/cov.hip, re-derived with the restated rule, and the properties they are there for."""
    plans = [R.slab_plan(c) for c in R.TABLE]
    assert [R.s_col(k) for k in (288, 516, 1020, 1032, 1548, 3276)] == [36, 64, 64, 65, 128, 218]
    assert [(p.slabs, p.per, p.last) for p in plans] == [(504, 2, 2), (896, 2, 2), (896, 2, 2), (845, 2, 1), (1755, 4, 3), (1792, 4, 4), (3052, 6, 4), (6104, 12, 8)]
    assert all(p.gx <= 512 and p.per % 2 == 0 and (p.gx - 1) * p.per < p.slabs <= p.gx * p.per for p in plans)
    assert any(p.per == 2 for p in plans) and any(p.per > 2 for p in plans)
    assert any(p.last == 1 for p in plans), "a last workgroup holding a single slab"
    assert any(p.last >= 3 and p.last % 2 == 1 for p in plans), "a last workgroup holding an odd count of at least 3"
    assert any(p.s_col % p.per for p in plans), "slab pairs that straddle symbol columns"
    assert plans[0].partner_rows == 0 and plans[1].partner_rows == 4 and plans[5].partner_rows == 12
    assert plans[2].partner_rows == 508 and plans[2].partner_ends_inside_slab and 508 // 8 == 63     # ends inside slab 63
    assert any(p.partner_ends_inside_slab for p in plans)
    assert any(p.masked_antennas for p in plans) and plans[1].masked_antennas == 15                  # ga + 32 >= 49 for ga = 17..31
    assert all(48 < c.n_ants <= 64 and 1 <= sum(c.los) <= 2 for c in R.TABLE)                        # the native route's own range
    assert any(c.los == (1, 0, 1) for c in R.TABLE) and any(c.los[0] == 0 for c in R.TABLE)
    assert plans[3].L_whole < plans[3].L_out and plans[4].L_whole < plans[4].L_out


def test_scene_builder_parameter_sets_agree():
    pkg = load_pkg()
    for case in tuple(R.TABLE) + tuple(R.NEIGHBOURS) + (R.BAND_CASE,):
        sc = R.build_scene(case, pkg.sensing.radarParams)
        got, want = sc.rp, sc.orp
        assert got.nIFFT == want.nIFFT == 4096 and got.nFFT == want.nFFT == (32 if case.n_sym == 14 else 64) and got.Pfa == want.Pfa == case.pfa
        for f in ("fc", "fs", "Tsri", "N0", "nIFFT", "nFFT", "rRes", "vRes", "rMax", "vMax", "Pfa", "nTxAnts", "nTargets", "txPower"):
            assert getattr(got, f) == getattr(want, f), f
        for f in ("range", "velocity", "largeScaleFading", "snrdB", "RxSteeringVec", "cfarEstZone"):
            assert np.array_equal(getattr(got, f), getattr(want, f)), f
        cg, cw = pkg.sensing.detection.cfar2D(got), O.cfar2d_config(want)
        assert np.array_equal(cg.CUTIdx, cw.CUTIdx) and cg.cfarDetector2D.ProbabilityFalseAlarm == cw.Pfa
        assert cg.cfarDetector2D.GuardBandSize == cw.GuardBandSize and cg.cfarDetector2D.TrainingBandSize == cw.TrainingBandSize
        assert (R.cfar_config(sc).GuardBandSize, R.cfar_config(sc).TrainingBandSize) == case.bands and (case.bands == R.DEFAULT_BANDS) == (case is not R.BAND_CASE)
        plan = R.slab_plan(case)
        assert (sc.K, sc.L_whole, sc.L_out, sc.A) == (plan.K, plan.L_whole, plan.L_out, case.n_ants) and sc.tx_grid.shape == (sc.K, sc.L_out, sc.A)


@pytest.mark.parametrize("case", R.TABLE, ids=lambda c: c.name)
def test_oracle_accepts_the_overridden_set(case):
    """O.fft2d runs on the overridden parameter set at every K of the table (the CUT window of the 4096-row map, the 32 / 64-point Doppler axis)."""
    o = _oracle_on_reference(case)
    sc = R.reference_of(case)[0]
    assert o.rdm.shape == (4096, sc.orp.nFFT, sc.A) and o.Ra.shape == (sc.A, sc.A) and len(o.detections) == sc.A


@pytest.mark.parametrize("case", [R.TABLE[1], R.TABLE[4], R.TABLE[5]], ids=lambda c: c.name)
def test_reference_echo_and_covariance_against_the_oracle(case):
    sc, e, ra, m, eta = R.reference_of(case)
    clean = R.reference_echo(sc, with_noise=False)
    want = O.mono_static_sensing(sc.tx_wave, sc.tx_grid.shape, sc.carrier, sc.orp, sc.los, None, nfft=4096)
    assert clean.shape == want.shape == (sc.K, sc.L_out, sc.A) and float(np.abs(clean - want).max()) <= 1e-10 * float(np.abs(want).max())
    # the noise the reference added is the restated Philox field of the stored grid, column l + L_out a, and nothing in the padding
    w = O.philox_spectral_noise(sc.K, sc.L_out, sc.A, case.noise_seed)
    nz = (e - clean) / R.noise_sigma(sc)
    assert float(np.abs(nz[:, :sc.L_whole, :] - w[:, :sc.L_whole, :]).max()) < 1e-9 and not e[:, sc.L_whole:, :].any()
    assert abs(float(nz[:, :sc.L_whole, :].real.std()) - 1) < 0.02 and abs(float(nz[:, :sc.L_whole, :].imag.std()) - 1) < 0.02
    want_ra = O.covariance(e)
    assert float(np.abs(ra - want_ra).max()) <= 1e-12 * float(np.abs(want_ra).max())
    g = e.reshape(-1, sc.A, order="F")
    assert np.allclose(m, np.abs(g).mean(axis=0), rtol=0, atol=0) and m.shape == (sc.A,) and eta > 0
    assert eta < 1e-6 * float(np.abs(e).max())                      # the element bound is a bound: seven digits below the grid's scale


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_guards_hold_on_the_reference_grid_with_a_decade_to_spare(case):
    o = _oracle_on_reference(case)
    assert o.cfar_margin > 1e-6, f"{case.name}: a CUT cell within {o.cfar_margin:.2e} of its threshold"
    assert o.eig_gap > 1e-8, f"{case.name}: eigenvalue gap {o.eig_gap:.2e} w[0] at the signal / noise split"
    assert (o.est is None) == (o.n_det == 0)


def test_band_case_is_asymmetric_and_detects():
    """The one lazy CPI at other bands: the default-band instance of every assertion above stays (the table, the neighbours, the sweep); this case differs from them in both
    half sizes, in both dimensions' order, keeps its window inside the map and has detections on most antennas."""
    case = R.BAND_CASE
    assert all(c.bands == R.DEFAULT_BANDS == ((2, 2), (1, 1)) for c in ALL_CASES if c is not case)
    (gr, gc), (tr, tc) = case.bands
    hr, hc = gr + tr, gc + tc
    assert (case.nrb, case.n_ants, len(case.targets), case.n_sym) == (25, 49, 1, 14) and gr != gc and hr != hc and min(gr, gc, tr, tc) >= 1 and hr != 3 and hc != 3
    o = _oracle_on_reference(case)
    sc = R.reference_of(case)[0]
    assert o.cfg.rowRange[0] - hr >= 1 and o.cfg.rowRange[1] + hr <= 4096 and o.cfg.colRange[0] - hc >= 1 and o.cfg.colRange[1] + hc <= sc.orp.nFFT
    assert sum(d.shape[1] > 0 for d in o.detections) > sc.A // 2 and o.n_det > sc.A and o.est is not None and 1 <= o.est.rngEst.size < sc.A


def test_enough_scenes_have_a_detection():
    """A run that compares only empty lists proves little: at least six of the eight table cases and at least four of the six sweep scenes have a detection."""
    table = [_oracle_on_reference(c).n_det > 0 for c in R.TABLE]
    sweep = [_oracle_on_reference(R.sweep_case(s)).n_det > 0 for s in R.SWEEP_SEEDS]
    assert sum(table) >= 6, table
    assert sum(sweep) >= 4, sweep
    # ... and a scene without one is there too: NO_DETECTION on both sides is part of the contract
    assert not all(table)
