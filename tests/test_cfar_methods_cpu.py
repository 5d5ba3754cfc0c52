"""The GOCA / SOCA / OS detectors (include/isac_cfar.h; project-defined) without a GPU: the additive header against the binding, the host-only
threshold factor against false-alarm expressions written out here, the NumPy restatement (tests/_cfar_methods_restatement.py) against the oracle's CA, a Monte-Carlo of
its false-alarm rate, the two-target scene the detectors exist for, and the conditioning of the scene x method pairs tests/test_gpu_cfar_methods.py runs as a chain."""
from __future__ import annotations

import ctypes
import math
import os
import re

import numpy as np
import pytest

import oracle as O
from conftest import ROOT, load_pkg

import _cfar_methods_restatement as M
import _target_list_restatement as R

CA, GOCA, SOCA, OS = 0, 1, 2, 3


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    return load_pkg()._lib


def _factor(L, method, n, rank, pfa):
    a = ctypes.c_double(float("nan"))
    st = L.load().isac_cfar_threshold_factor(method, n, rank, pfa, ctypes.byref(a))
    return st, a.value


def test_header_against_the_binding(L):
    """isac_cfar.h is additive under ABI 8; the struct's size agrees through its isac_abi_sizeof selector, 12 of ABI_STRUCTS, and the method constants are the
    binding's.  (Its prototype lines are compared with the header by tests/test_abi_cpu.py, row "isac_cfar.h".)"""
    hdr = open(os.path.join(ROOT, "include", "isac_cfar.h")).read()
    assert L.ISAC_ABI_VERSION == 8
    plain = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    lib = L.load()                                                             # (needs no GPU) load() checked the struct size
    sel = int(re.search(r"#define ISAC_SIZEOF_CFAR_METHOD (\d+)", hdr).group(1))
    assert sel == 12 and L.ABI_STRUCTS[sel] == ("isac_cfar_method", L.CfarMethod)
    assert lib.isac_abi_sizeof(sel) == ctypes.sizeof(L.CfarMethod) == 16 and lib.isac_abi_version() == 8
    consts = {n: int(v) for n, v in re.findall(r"\bISAC_CFAR_(CA|GOCA|SOCA|OS) = (\d+)", plain)}
    assert consts == {"CA": L.CFAR_CA, "GOCA": L.CFAR_GOCA, "SOCA": L.CFAR_SOCA, "OS": L.CFAR_OS} == L.CFAR_METHODS
    assert int(re.search(r"#define ISAC_CFAR_MAX_TRAIN (\d+)", hdr).group(1)) == L.ISAC_CFAR_MAX_TRAIN


# ---- the false-alarm expressions of the issue, written out with exact binomials (not the library's ratio recurrence)
def _soca(n, T):
    return 2.0 * math.fsum(math.comb(n - 1 + k, k) * (2.0 + T) ** -(n + k) for k in range(n))


def _pfa(method, N, alpha, rank):
    n = N // 2
    if method == SOCA:
        return _soca(n, alpha / n)
    if method == GOCA:
        return 2.0 * (1.0 + alpha / n) ** -n - _soca(n, alpha / n)
    return math.prod((N - i) / (N - i + alpha) for i in range(rank))


def test_ca_factor_is_the_closed_form_bitwise(L):
    for N in (1, 2, 8, 24, 416, 5000):
        for pfa in (1e-1, 1e-2, 1e-6, 1e-9):
            st, a = _factor(L, CA, N, 0, pfa)
            assert st == 0 and a == O.cfar.cfar_threshold_factor(N, pfa) == N * (pfa ** (-1.0 / N) - 1.0)


@pytest.mark.parametrize("N", [2, 8, 24, 416])
@pytest.mark.parametrize("pfa", [1e-1, 1e-2, 1e-6])
def test_solved_factor_reproduces_pfa(L, N, pfa):
    """Substituting the returned alpha gives Pfa within 1e-10 relative (the project's field tolerance) for every method, OS at ranks 1, N/2, ceil(3N/4), N."""
    worst = 0.0
    for method, ranks in ((GOCA, (0,)), (SOCA, (0,)), (OS, sorted({1, N // 2, math.ceil(3 * N / 4), N}))):
        for rank in ranks:
            st, a = _factor(L, method, N, rank, pfa)
            assert st == 0 and a > 0.0
            rel = abs(_pfa(method, N, a, rank) / pfa - 1.0)
            worst = max(worst, rel)
            assert rel <= 1e-10, (method, rank, a, rel)
            # the restatement's solver: the same algorithm, so both are ends of a one-ulp bracket of the root -- of functions whose rounding (~1e-14) may differ
            assert abs(a / M.threshold_factor(M.METHODS[method], N, pfa, rank) - 1.0) <= 1e-12
    print(f"N = {N}, Pfa = {pfa}: worst relative error {worst:.2e}")


def test_worked_values_and_n2(L):
    got = [_factor(L, m, 24, 18, 1e-2)[1] for m in (CA, SOCA, GOCA, OS)]
    print("N = 24, Pfa = 1e-2, rank 18: CA, SOCA, GOCA, OS =", got)
    for g, want in zip(got, (5.07666, 6.40866, 4.46236, 4.02538)):
        assert abs(g - want) < 1e-5                                             # the five decimals the issue gives, truncated
    soca, os1 = _factor(L, SOCA, 2, 0, 1e-2)[1], _factor(L, OS, 2, 1, 1e-2)[1]
    assert abs(soca / 198.0 - 1.0) <= 1e-10 and abs(os1 / 198.0 - 1.0) <= 1e-10 and abs(soca / os1 - 1.0) <= 1e-10


def test_bad_arguments_are_refused(L):
    INVALID, UNSUPPORTED = 1, 7
    nan = float("nan")
    for method, n, rank, pfa in ((4, 24, 1, 1e-2), (-1, 24, 1, 1e-2),                       # unknown method
                                 (OS, 24, 0, 1e-2), (OS, 24, 25, 1e-2), (OS, 24, -3, 1e-2),  # rank outside 1..N
                                 (CA, 0, 1, 1e-2), (SOCA, 0, 1, 1e-2), (OS, -2, 1, 1e-2),    # no training cell
                                 (GOCA, 7, 1, 1e-2), (SOCA, 7, 1, 1e-2),                     # halves of an odd N
                                 (CA, 24, 1, 0.0), (GOCA, 24, 1, 1.0), (SOCA, 24, 1, -0.1), (OS, 24, 1, 1.5), (OS, 24, 1, nan), (CA, 24, 1, nan)):
        assert _factor(L, method, n, rank, pfa)[0] == INVALID, (method, n, rank, pfa)
    for method in (GOCA, SOCA, OS):
        assert _factor(L, method, L.ISAC_CFAR_MAX_TRAIN + 2, 1, 1e-2)[0] == UNSUPPORTED
        assert _factor(L, method, L.ISAC_CFAR_MAX_TRAIN, 1, 1e-2)[0] == 0
    assert L.load().isac_cfar_threshold_factor(CA, 24, 1, 1e-2, None) == INVALID
    pkg = load_pkg()
    assert pkg.sensing.detection.cfarThresholdFactor("OS", 24, 1e-2, Rank=18) == _factor(L, OS, 24, 18, 1e-2)[1]
    with pytest.raises(pkg.IsacError):
        pkg.sensing.detection.cfarThresholdFactor("OS", 24, 1e-2, Rank=25)
    with pytest.raises(ValueError):
        pkg.sensing.detection.cfarThresholdFactor("XX", 24, 1e-2)


def test_restatement_ca_equals_the_oracle():
    rng = np.random.default_rng(3)
    P = rng.exponential(size=(40, 36))
    P[20, 18], P[9, 30] = 400.0, 90.0
    for guard, train in (((2, 2), (1, 1)), ((0, 0), (1, 1)), ((1, 0), (2, 1)), ((0, 1), (1, 0))):
        hr, hc = guard[0] + train[0], guard[1] + train[1]
        cuts = M.rectangle_cuts((hr + 1, 40 - hr, hc + 1, 36 - hc))
        N = M.n_train(guard, train)
        assert N == (2 * hr + 1) * (2 * hc + 1) - (2 * guard[0] + 1) * (2 * guard[1] + 1) and N % 2 == 0
        want, thr_o = O.cfar.ca_cfar2d(P, cuts, 1e-2, guard, train, return_threshold=True)
        got, thr = M.detect(P, cuts, guard, train, "CA", M.threshold_factor("CA", N, 1e-2), return_threshold=True)
        assert np.array_equal(got, want) and thr.tobytes() == thr_o.tobytes() and want.shape[1] >= 2
        # the front half of the order is the cells before the CUT in column-major order
        offs = O.cfar.training_offsets(guard, train)
        assert all((dc, dr) < (0, 0) for dr, dc in offs[: N // 2]) and all((dc, dr) > (0, 0) for dr, dc in offs[N // 2:])


@pytest.mark.parametrize("N,rank", [(24, 18), (8, 6), (2, 1)])
def test_monte_carlo_false_alarm_rate(N, rank):
    """400 000 independent exponential draws per case, Pfa = 1e-2: each method's rate within 5 sigma, sigma = sqrt(Pfa (1 - Pfa) / n) = 1.57e-4.  A mean / sum or a
    half / whole mistake moves the rate by orders of magnitude."""
    n, pfa = 400_000, 1e-2
    rng = np.random.default_rng(1)
    T = rng.exponential(size=(N, n))
    cut = rng.exponential(size=n)
    sigma = math.sqrt(pfa * (1.0 - pfa) / n)
    for method in M.METHODS:
        alpha = M.threshold_factor(method, N, pfa, rank)
        rate = float(np.mean(cut > alpha * M.noise_estimate(T, method, rank)))
        print(f"N = {N}, {method}{f' rank {rank}' if method == 'OS' else ''}: alpha {alpha:.6f}, rate {rate:.6f} = Pfa {(rate - pfa) / sigma:+.2f} sigma")
        assert abs(rate - pfa) <= 5.0 * sigma, (method, rate)


def test_nan_rule_and_ties():
    P = np.ones((9, 9))
    P[4, 4] = 1e6
    cuts = np.array([[5], [5]])
    for method, rank in (("CA", 1), ("GOCA", 1), ("SOCA", 1), ("OS", 1), ("OS", 24)):
        assert M.detect(P, cuts, (2, 2), (1, 1), method, 2.0, rank).shape[1] == 1               # a plateau of equal training cells: every rank gives 1.0
        for cell in ((1, 1), (7, 7), (1, 4)):                                                  # front half, rear half, front half of the centre column
            Q = P.copy()
            Q[cell] = np.nan
            assert M.detect(Q, cuts, (2, 2), (1, 1), method, 2.0, rank).shape[1] == 0
        Q = P.copy()
        Q[4, 4] = np.nan
        assert M.detect(Q, cuts, (2, 2), (1, 1), method, 2.0, rank).shape[1] == 0
        Q = P.copy()
        Q[3, 3] = np.nan                                                                       # inside the guard block: not a training cell
        assert M.detect(Q, cuts, (2, 2), (1, 1), method, 2.0, rank).shape[1] == 1


def test_two_targets_one_in_the_others_training_band():
    """What the detectors are for.  An exponential floor, a strong target and a weaker one three rows below it: each sits in the other's training band (guard 2,
    training 1).  CA and GOCA lose the weaker target; SOCA (the clean half) and OS (one interferer among 24 cells, rank 18) detect both."""
    rng = np.random.default_rng(7)
    P = rng.exponential(size=(40, 36))
    strong, weak = (20, 18), (23, 18)                                                          # 1-based
    P[strong[0] - 1, strong[1] - 1], P[weak[0] - 1, weak[1] - 1] = 1e4, 300.0
    cuts = np.array([strong, weak]).T
    got = {}
    for method in M.METHODS:
        alpha = M.threshold_factor(method, 24, 1e-3, 18)
        d, thr = M.detect(P, cuts, (2, 2), (1, 1), method, alpha, 18, return_threshold=True)
        got[method] = [tuple(x) for x in d.T.tolist()]
        print(f"{method}: alpha {alpha:.4f}, thresholds {thr.tolist()}, detected {got[method]}")
    assert got["SOCA"] == [strong, weak] and got["OS"] == [strong, weak]
    assert got["CA"] == [strong] and got["GOCA"] == [strong]


def test_chain_pairs_clear_the_guard_band():
    """Every scene x method pair of the GPU chain test on the oracle's power window: every CUT's |P - thr| / thr must exceed 1e-9.  Pairs that do not are dropped from
    the GPU chain test (it asks chain_pairs() too) and named here; at most one may be."""
    cleared, dropped = M.chain_pairs()
    for name, method, rank in cleared + dropped:
        r = M.oracle_redetect(name, method, rank)
        print(f"{name} {method}: margin {r.margin:.3e}, {r.totalDetections} detections, numDets {r.numDets}{'  DROPPED' if (name, method, rank) in dropped else ''}")
    assert len(cleared) + len(dropped) == len(R.SCENES) * len(M.CHAIN_METHODS)
    assert len(dropped) <= 1, dropped
    # the scene at other bands than the default: every method cleared (nothing of it is dropped at run time), asymmetric, 78 training cells that split into halves
    guard, train = R.bands_of(R.BAND_SCENE)
    assert (guard, train) == R.READER_BANDS != R.DEFAULT_BANDS == (M.GUARD, M.TRAIN) and M.n_train(guard, train) == 78
    assert guard[0] != guard[1] and guard[0] + train[0] != guard[1] + train[1] and min(guard[0] + train[0], guard[1] + train[1]) >= 1
    assert [p for p in cleared if p[0] == R.BAND_SCENE] == [(R.BAND_SCENE, m, k) for m, k in M.chain_methods(R.BAND_SCENE)] and M.chain_methods(R.BAND_SCENE)[3] == ("OS", 58)
    assert all(M.chain_methods(n) == M.CHAIN_METHODS for n in R.SCENES if n != R.BAND_SCENE)
    assert all(M.oracle_redetect(R.BAND_SCENE, m, k).totalDetections > 0 for m, k in M.chain_methods(R.BAND_SCENE))
    # CA on the oracle window is the oracle's own fft2D
    for name in R.SCENES:
        t, r = R.oracle_targets(name), M.oracle_redetect(name, "CA", 1)
        assert np.array_equal(r.rngEst, t.est.rngEst) and np.array_equal(r.velEst, t.est.velEst)
    assert any(M.oracle_redetect(n, m, k).totalDetections > 0 for n, m, k in cleared if m != "CA")
