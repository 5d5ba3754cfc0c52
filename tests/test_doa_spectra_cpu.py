"""The ULA DoA spectra of MUSIC, digitalBF and mvdrBF value by value, on the CPU: the oracle (oracle.music.music_spectrum_ula / digital_bf / mvdr_bf) and the
eigen-weighted fp64 restatement of music_scan_kernel (tests/_doa_reference.restatement, plus oracle.subspace_music.music_spectrum_subspace for the
signal-subspace route) against the extended-precision reference of tests/_doa_reference.py, on every case tests/test_gpu_doa_spectra.py runs on the device.

* Condition on the inputs: both fp64 formulations stay within TOL_FP64 = 1e-8 dB of the reference at every scan point of every case -- 100 x inside the
  device tolerance of the GPU file.  The cases keep cond(Ra) <= 1e7 (MVDR), a gap >= 1e-3 w[0] at every signal / noise split that is scanned and
  min a'Uan Uan'a >= 1e-6 A (MUSIC); all three are asserted here.
* Sensitivity: the comparison that the GPU file applies (deviation <= TOL_DB = 1e-6 dB, finite where the reference lies above -200 dB) rejects every
  mutant of the restatement in _doa_reference.MUTANTS on at least one committed case, and accepts the unmutated restatement on all of them.  Removing
  `+ eps` from the quadratic forms is not among them: under the floor above it moves a value by at most 8.7 eps / (1e-6 A) ~ 2e-9 dB, below the
  resolution of the comparison by construction.
"""
from __future__ import annotations

import numpy as np
import pytest

import _doa_reference as R
from oracle import music as M
from oracle import subspace_music as SM
from oracle.matlab_compat import findpeaks

TOL_FP64 = 1e-8     # dB: the two fp64 formulations against the reference
TOL_DB = 1e-6       # dB: the device tolerance (tests/test_gpu_doa_spectra.py), what the mutants must exceed
RP = R.rp_ula()


def _check_conditions(w_desc, y, n_sig, a):
    """The MUSIC input conditions of the module docstring at one split (nothing to check for an empty noise space)."""
    if n_sig >= a:
        return
    w = R._f64(w_desc)
    assert w[n_sig - 1] - w[n_sig] >= 1e-3 * w[0], ("gap", a, n_sig)
    assert float(R._f64(y[n_sig:].sum(axis=0)).min()) >= 1e-6 * a, ("floor", a, n_sig)


def _fp64_formulations(method, ra, n_sig):
    """(name, dB spectrum) of every fp64 statement of one method: the oracle's, the kernel's eigen-weighted sums and, for MUSIC, the subspace
    route's || a - Us Us' a ||^2."""
    a = ra.shape[0]
    if method == 0:
        n_ret, _, _, pdb = M.music_doa(n_sig, RP, ra, return_db=True)       # (= music_spectrum_ula on _noise_projector's Uan Uan')
        assert n_ret == n_sig
        w, v = np.linalg.eigh(ra)
        us = v[:, np.argsort(-w, kind="stable")[:min(n_sig, a)]]
        return [("oracle", pdb), ("restatement", R.restatement(0, ra, n_sig)), ("subspace", SM.music_spectrum_subspace(us, a, RP))]
    fn = M.digital_bf if method == 1 else M.mvdr_bf
    return [("oracle", fn(2, RP, ra, return_db=True)[2]), ("restatement", R.restatement(method, ra))]


@pytest.mark.parametrize("a", R.ARRAY_SIZES)
def test_prescribed_eigenstructure(a, record_property):
    worst = {0: 0.0, 1: 0.0, 2: 0.0}
    y = R.prescribed_projections(a)
    for spread in (R.SPREADS if a > 1 else R.SPREADS[:1]):
        c = R.prescribed_case(a, spread)
        w = R._f64(c.w)
        assert a == 1 or abs(w[0] / w[-1] / spread - 1) < 1e-12            # cond(Ra) = the spread, <= 1e7
        for method in (1, 2):
            ref = R.prescribed_spectrum(c, method)
            for name, got in _fp64_formulations(method, c.ra, None):
                d = R.deviation(got, ref)
                worst[method] = max(worst[method], d)
                assert d <= TOL_FP64, (a, spread, method, name, d)
        for n_sig in (R.music_num_dets(a, c.n_src) if spread == R.MUSIC_SPREAD or a == 1 else [max(c.n_src, 1)]):
            _check_conditions(c.w, y, n_sig, a)
            ref = R.prescribed_spectrum(c, 0, n_sig)
            if n_sig >= a:
                assert np.all(ref == 0.0)                                   # empty noise space: flat
            for name, got in _fp64_formulations(0, c.ra, n_sig):
                d = R.deviation(got, ref)
                worst[0] = max(worst[0], d)
                assert d <= TOL_FP64, (a, spread, n_sig, name, d)
    for method, name in ((0, "music"), (1, "dbf"), (2, "mvdr")):
        record_property(f"fp64_vs_reference_db_{name}", worst[method])


@pytest.mark.parametrize("name", sorted(R.PHYSICAL))
def test_physical_covariances(name):
    """Sample covariances of off-grid sources plus noise against mpmath's eighe / inverse at 40 digits; the prescribed-structure reference and the
    sign-function projector agree with it on the same matrix."""
    c = R.physical_case(name)
    w = R._f64(c.w)
    assert w[0] / w[-1] <= 1e7
    y = R.projections(c.v, R.scan_angles())
    for method in (1, 2):
        ref = R.physical_spectrum(c, method)
        assert R.deviation(R.spectra_from_projections(c.w, y, method), ref) <= 1e-12      # eigen-weighted sums == a'Ra a, a'Ra^-1 a (both extended)
        for nm, got in _fp64_formulations(method, c.ra, None):
            assert R.deviation(got, ref) <= TOL_FP64, (name, method, nm)
    for n_sig in (1, c.n_src):
        _check_conditions(c.w, y, n_sig, c.A)
        ref = R.physical_spectrum(c, 0, n_sig)
        assert R.deviation(R.sign_projector_music(c.ra, n_sig), ref) <= 1e-11
        for nm, got in _fp64_formulations(0, c.ra, n_sig):
            assert R.deviation(got, ref) <= TOL_FP64, (name, n_sig, nm)


def test_non_default_scans():
    """The two grids the GPU file scans after the default one: 362 steps of 0.5 degrees over +-90 (none AT +-90: -90 ... 90.5 is the music.m:79,88 grid),
    180 steps of 2 degrees."""
    c = R.prescribed_case(16, R.MUSIC_SPREAD)
    for gran, scale, steps in ((0.5, 180.0, 362), (2.0, 360.0, 180)):
        ang = R.scan_angles(gran, scale)
        assert ang.size == steps
        rp = R.rp_ula(gran, scale)
        for method in (0, 1, 2):
            ref = R.prescribed_spectrum(c, method, c.n_src, gran, scale)
            got = (M.music_doa(c.n_src, rp, c.ra, return_db=True)[3] if method == 0 else
                   (M.digital_bf if method == 1 else M.mvdr_bf)(2, rp, c.ra, return_db=True)[2])
            assert ref.size == steps and R.deviation(got, ref) <= TOL_FP64
            assert R.deviation(R.restatement(method, c.ra, c.n_src, gran, scale), ref) <= TOL_FP64
    assert R.scan_angles(0.5, 180.0)[0] == -90.0 and R.scan_angles(0.5, 180.0)[-1] == 90.5


def test_three_methods_give_three_peak_lists():
    """Two sources 3 degrees apart at A = 16: the reference's own peak lists differ pairwise (a swap of the methods changes the estimates, not only the
    values); the oracle's lists equal the reference's."""
    c = R.physical_case("close3")
    lists = []
    for method in (0, 1, 2):
        _, locs = findpeaks(R.physical_spectrum(c, method, 2), npeaks=2)
        lists.append(tuple(locs - 180.0))
    assert len(set(lists)) == 3, lists
    assert tuple(M.music_doa(2, RP, c.ra)[1]) == lists[0] and tuple(M.digital_bf(2, RP, c.ra)[0]) == lists[1] and tuple(M.mvdr_bf(2, RP, c.ra)[0]) == lists[2]


def _mutant_cases():
    for a in (16, 256):
        c = R.prescribed_case(a, R.MUSIC_SPREAD)
        yield f"prescribed{a}", c.ra, c.n_src, lambda m, c=c: R.prescribed_spectrum(c, m, c.n_src)
    c = R.physical_case("a16")
    yield "a16", c.ra, c.n_src, lambda m, c=c: R.physical_spectrum(c, m, c.n_src)


def test_unmutated_restatement_is_accepted():
    for name, ra, n_sig, ref in _mutant_cases():
        for method in (0, 1, 2):
            assert R.accept(R.restatement(method, ra, n_sig), ref(method), TOL_DB), (name, method)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_comparison_rejects_mutant(mutant):
    rejected = [(name, method) for name, ra, n_sig, ref in _mutant_cases() for method in (0, 1, 2)
                if not R.accept(R.restatement(method, ra, n_sig, mutant=mutant), ref(method), TOL_DB)]
    assert rejected, mutant
    # the methods a mutation does not touch still pass (the rejection is the mutation's, not the harness's)
    touched = {"swap_dbf_mvdr": (1, 2), "mvdr_weighted_by_w": (2,), "L_plus_1": (0,), "L_minus_1": (0,)}.get(mutant, (0, 1, 2))
    assert all(method in touched for _, method in rejected), (mutant, rejected)


def test_reference_building_blocks():
    """sind exact at the multiples of 90 and mirror-symmetric; steering vectors of unit modulus; the deviation helper refuses non-finite values where the
    reference is finite and lets equal infinities pass."""
    s = R._f64(R.sind_ext(np.array([-180.0, -90.0, 0.0, 90.0, 180.0, 30.0, 150.0])))
    assert np.array_equal(s[:5], [0.0, -1.0, 0.0, 1.0, 0.0]) and s[5] == s[6] and abs(s[5] - 0.5) < 1e-16
    assert np.abs(R._f64(R._abs2(R.steering(7, R.scan_angles()))) - 1.0).max() < 1e-18
    ref = np.array([0.0, -10.0, -np.inf])
    assert R.accept(np.array([0.0, -10.0, -np.inf]), ref, TOL_DB)
    assert not R.accept(np.array([0.0, np.nan, -np.inf]), ref, TOL_DB) and not R.accept(np.array([0.0, -10.0, -300.0]), ref, TOL_DB)
