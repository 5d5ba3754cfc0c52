"""music2D's range and velocity spectra value by value, on the CPU: what tests/test_gpu_music2d_spectra.py relies on.

* Route agreement: the reference's own route in mpmath (eig of the K x K Rr and of the Ls x Ls Rv, 1 / (a' Un Un' a)) and the extended-precision route
  through the smaller Gram matrix with the residual 1 / |a - Us Us' a|^2 (tests/_music2d_reference.py) agree to 1e-12 dB on the small cases.
* Condition of every case that runs on the device: the fp64 statement of the reference's formulation (_music2d_reference.restatement, and the oracle's
  music2d where K <= 512) stays within TOL_FP64 = 1e-8 dB of the reference at every scan point -- 100 x inside the device tolerance, the condition
  tests/test_doa_spectra_cpu.py imposes on the ULA cases.  determineNumTargets on the case's Ra gives the intended L (with the smallest eigenvalue gap
  at most half of the next: asserted where the case is made).
* Sensitivity: the comparison of the GPU file (deviation <= TOL_DB = 1e-6 dB, finite where the reference lies above -200 dB) rejects every mutant of
  _music2d_reference.MUTANTS on at least one case and accepts the unmutated statements of the reference's and of the device's formulation on all.
* The formulation music2d_scan_kernel had before this comparison, 1 / (N - sum_i |u_i' a|^2), is NOT accepted: on the 100 dB cases with targets on the
  scan grid it leaves the tolerance by orders of magnitude (the difference of two numbers of size N), which is why the kernel sums the residual.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest

import _music2d_reference as M
from oracle import music as OM
from oracle.matlab_compat import findpeaks

TOL_FP64 = 1e-8
TOL_DB = M.TOL_DB
SMALL = M.CASES["base"] + M.CASES["K_lt_Ls"] + [M.EMPTY_NOISE_SPACE]
EVERY = [args for _, args in M.ALL_CASES] + [M.EMPTY_NOISE_SPACE]
# one case per code path of the restatement: L = 3 at 30 dB, 100 dB on the grid, K < Ls, K = 65 and Ls = 65 (a second wave in either sum), K = 257
MUTANT_CASES = [M.CASES["base"][1], M.CASES["base"][4], M.CASES["K_lt_Ls"][1], M.CASES["wave"][4], M.CASES["Ls65"][0], M.CASES["block"][5]]


def _dev(got, ref):
    return max(M.deviation(got[0][ref.r_idx], ref.PrdB), M.deviation(got[1][ref.v_idx], ref.PvdB))


def _accept(got, ref):
    return M.accept(got[0][ref.r_idx], ref.PrdB, TOL_DB) and M.accept(got[1][ref.v_idx], ref.PvdB, TOL_DB)


@pytest.mark.parametrize("args", SMALL, ids=M.case_id)
def test_route_agreement(args):
    ref = M.reference(args)
    pr, pv = M.full_route_mp(args)
    d = _dev((pr, pv), ref)
    print(f"{M.case_id(args)}: full K x K mpmath route against the Gram route {d:.2e} dB")
    assert ref.r_idx.size == pr.size and ref.v_idx.size == pv.size and d <= 1e-12


@pytest.mark.parametrize("args", EVERY, ids=M.case_id)
def test_condition_of_the_case(args, record_property):
    c = M.make_case(*args)
    ref = M.reference(args)
    assert OM.determine_num_targets(np.linalg.eigvalsh(0.5 * (c.Ra + c.Ra.conj().T))) == c.L
    steps = (M.grids()[0].size, M.grids()[1].size)
    assert 100 <= steps[0] <= 250 and 100 <= steps[1] <= 250
    d = _dev(M.restatement(args, "reference"), ref)
    record_property("fp64_reference_form_db", d)
    print(f"{M.case_id(args)}: fp64 statement of the reference's formulation {d:.2e} dB")
    assert d <= TOL_FP64
    if c.K <= 512 and c.L < c.Ls:                           # the oracle (a NaN spectrum where the noise space is empty: its own convention)
        est, dbg = OM.music2d(c.rp, M.SCS_KHZ, c.rx, c.tx, return_debug=True)
        assert dbg.L == c.L and _dev((dbg.PrdB, dbg.PvdB), ref) <= TOL_FP64
        full = ref.r_idx.size == steps[0]
        assert not full or np.array_equal(est.rngEst, findpeaks(ref.PrdB, npeaks=c.L)[1] * M.GRAN)


def test_empty_noise_space_is_flat():
    ref = M.reference(M.EMPTY_NOISE_SPACE)
    assert ref.case.L >= ref.case.Ls and np.all(ref.PvdB == 0.0) and findpeaks(ref.PvdB, npeaks=ref.case.L)[1].size == 0
    assert ref.PrdB.min() < -20.0 and np.all(np.isfinite(ref.PrdB))


def test_unmutated_statements_are_accepted():
    for args in EVERY:
        if args[0] > 512:
            continue                                        # (the K x K eig of the named K: once, in test_condition_of_the_case)
        ref = M.reference(args)
        for form in ("reference", "gram_residual"):
            assert _accept(M.restatement(args, form), ref), (M.case_id(args), form)
    for args in M.CASES["named_K"]:
        assert _accept(M.restatement(args, "gram_residual"), M.reference(args)), M.case_id(args)


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_comparison_rejects_mutant(mutant):
    rejected = [M.case_id(args) for args in MUTANT_CASES if not _accept(M.restatement(args, "gram_residual", mutant=mutant), M.reference(args))]
    print(f"{mutant}: rejected on {len(rejected)} of {len(MUTANT_CASES)} cases")
    assert rejected, mutant


def test_difference_of_two_large_numbers_leaves_the_tolerance():
    worst = {}
    for grp in ("base", "block", "Ls65"):
        for args in M.CASES[grp]:
            worst[M.case_id(args)] = _dev(M.restatement(args, "gram_difference"), M.reference(args))
    on_grid_100 = [k for k in worst if "-100dB-s1" in k]
    print({k: f"{v:.1e}" for k, v in worst.items()})
    assert len(on_grid_100) == 3 and all(worst[k] > 10 * TOL_DB for k in on_grid_100)


def test_reference_building_blocks():
    """Steering vectors of unit modulus that agree with fp64's; the scan grids of music2D.m:45-46,99,105."""
    r, v = M.grids()
    assert r.size == 122 and v.size == 122 and r[0] == 0.0 and r[-1] == 60.5 and v[0] == -30.0 and v[-1] == 30.5
    for kind, x, n in (("r", r, 300), ("v", v, 65)):
        s = M._steer_ext(kind, x, n)
        assert np.abs(M._f64(M._abs2(s)) - 1.0).max() < 1e-18
        s64 = np.asarray(s if M.EXT else M.R._each(complex, s), dtype=np.complex128)
        assert np.abs(s64 - M.steer64(kind, x, n)).max() < 1e-12
    c = M.make_case(*M.CASES["base"][0])
    assert np.allclose(np.abs(c.tx), 1.0) and c.rx.flags.f_contiguous and isinstance(c.rp, SimpleNamespace)
