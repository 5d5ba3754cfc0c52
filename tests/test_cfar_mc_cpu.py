"""The sensing KPIs without a GPU: the additive header include/isac_cfar_mc.h against the binding, the NumPy restatement of the Monte Carlo
(tests/_cfar_mc_restatement.py) against the false-alarm / detection expressions, sensing.detection.getPd against SciPy, sensing.postProcessing.getRMSE case by case."""
from __future__ import annotations

import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
from scipy import special

from conftest import ROOT, load_pkg

import _cfar_methods_restatement as M
import _cfar_mc_restatement as MC


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    return load_pkg()._lib


def test_header_against_the_binding(L):
    """isac_cfar_mc.h is additive under ABI 8: no new isac_abi_sizeof selector, its target-model constants are the binding's, its one function refuses a NULL context.
    (Its prototype line is compared with the header by tests/test_abi_cpu.py, row "isac_cfar_mc.h".)"""
    hdr = open(os.path.join(ROOT, "include", "isac_cfar_mc.h")).read()
    assert L.ISAC_ABI_VERSION == 8
    plain = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    lib = L.load()                                                             # (needs no GPU)
    assert lib.isac_abi_version() == 8
    assert len(L.ABI_STRUCTS) == 13 and L.ABI_STRUCTS[11:] == (("isac_target_list", L.TargetList), ("isac_cfar_method", L.CfarMethod))
    assert lib.isac_abi_sizeof(13) == -1                                       # no new selector
    consts = {n: int(v) for n, v in re.findall(r"\bISAC_TARGET_(SW0|SW1) = (\d+)", plain)}
    assert consts == {"SW0": L.TARGET_SW0, "SW1": L.TARGET_SW1} and sorted(L.TARGET_MODELS.values()) == [0, 1]
    assert int(re.search(r"#define ISAC_CFAR_MC_MAX_TRAIN (\d+)", hdr).group(1)) == L.ISAC_CFAR_MC_MAX_TRAIN == 128
    # refused before anything touches a device: no context
    assert lib.isac_cfar_monte_carlo(None, None, 24, 1e-2, 0, None, 1, 1, 0, None, None) == 1


def test_restatement_against_the_expressions():
    """2^20 trials, N = 24, Pfa 1e-2, every method: the false-alarm count, and the Swerling 1 / Swerling 0 (CA) counts at 0, 5, 10 dB, within 5 sigma of the expressions;
    no (trial, SNR point) pair within 1e-12 of its threshold."""
    N, pfa, n, rank, seed = 24, 1e-2, 1 << 20, 18, 1
    snr = [-np.inf, 0.0, 5.0, 10.0]
    cases = [(m, M.threshold_factor(m, N, pfa, rank)) for m in M.METHODS]
    cnt = {(m, model): np.zeros(len(snr), dtype=np.int64) for m, _ in cases for model in MC.MODELS}
    closest = np.inf
    for t0 in range(0, n, 1 << 18):
        d = MC.draw(N, seed, 1 << 18, t0)
        for m, alpha in cases:
            for model in MC.MODELS:
                f, mg = MC.detect(d, m, rank, alpha, model, snr)
                cnt[(m, model)] += f.sum(axis=0, dtype=np.int64)
                closest = min(closest, float(mg.min()))
    print(f"closest (trial, SNR point) pair: margin {closest:.3e}")
    assert closest > 1e-12
    for m, alpha in cases:
        assert abs(MC.false_alarm(m, N, alpha, rank) / pfa - 1.0) < 1e-9
        want1 = np.concatenate([[pfa], MC.pd_swerling1(m, N, alpha, rank, snr[1:])])
        for model, want in (("swerling1", want1), ("swerling0", np.concatenate([[pfa], MC.pd_swerling0_ca(N, alpha, snr[1:])]) if m == "CA" else [pfa])):
            for i, p in enumerate(want):
                ok, z = MC.within_5_sigma(int(cnt[(m, model)][i]), n, float(p))
                print(f"{m} {model} {snr[i]} dB: {cnt[(m, model)][i]} of {n}, expected {p:.6e}, {z:+.2f} sigma")
                assert ok, (m, model, snr[i])
        assert (np.diff(cnt[(m, "swerling1")]) >= 0).all()                     # common random numbers


def test_restatement_is_a_function_of_seed_and_trial():
    a, b = MC.draw(8, 7, 100), MC.draw(8, 7, 40, t0=60)
    assert all(np.array_equal(x[..., 60:], y) for x, y in zip(a, b))
    assert not np.array_equal(MC.draw(8, 8, 100)[1], a[1])
    big = MC.draw(2, 7, 4, t0=(1 << 32) - 2)                                   # the counter's high word
    assert np.unique(big[1]).size == 4 and (big[0] > 0).all() and ((big[2] >= 0) & (big[2] < 2 * np.pi)).all()


# ---------------------------------------------------------------- getPd
@pytest.mark.parametrize("n_pulses", [1, 10])
def test_getPd_against_scipy(n_pulses):
    pkg = load_pkg()
    pfa, snr = np.array([1e-9, 1e-6, 1e-3]), np.linspace(-5.0, 20.0, 21)
    pd = pkg.sensing.detection.getPd(pfa, snr, n_pulses)
    want = 0.5 * special.erfc(special.erfcinv(2.0 * pfa)[None, :] - np.sqrt(n_pulses * 10.0 ** (snr / 10.0))[:, None])
    assert pd.shape == (21, 3)
    print("max |Pd - SciPy|:", np.abs(pd - want).max())
    assert np.abs(pd - want).max() <= 1e-12
    assert (np.diff(pd, axis=0) >= 0.0).all() and (pd > 0).all() and (pd <= 1).all()
    # only the ends and the count of snrdB are used (getPd.m:9-12)
    bent = snr.copy()
    bent[1:-1] = 3.0
    assert np.array_equal(pkg.sensing.detection.getPd(pfa, bent, n_pulses), pd)
    at0 = pkg.sensing.detection.getPd(pfa, [-300.0], n_pulses)
    assert at0.shape == (1, 3) and np.abs(at0[0] / pfa - 1.0).max() <= 1e-12
    assert pkg.sensing.detection.getPd(1e-3, [0.0, 10.0], n_pulses).shape == (2, 1)
    with pytest.raises(ValueError):
        pkg.sensing.detection.getPd(0.0, snr, n_pulses)


# ---------------------------------------------------------------- getRMSE
def _params(kind="ula", r_res=1.0):
    truth = [dict(ID=1, Range=100.0, Velocity=5.0, Elevation=2.0, Azimuth=30.0, snrdB=20.0), dict(ID=2, Range=140.0, Velocity=-3.0, Elevation=-4.0, Azimuth=-10.0, snrdB=10.0)]
    return SimpleNamespace(rRes=r_res, antennaType=SimpleNamespace(kind=kind), targetRealPos=truth)


def _eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b, dtype=np.float64), equal_nan=True)


def test_getRMSE_inside_and_outside_the_resolution_cell():
    g = load_pkg().sensing.postProcessing.getRMSE
    nan = math.nan
    est = SimpleNamespace(rngEst=[140.25, 100.5, 120.0], velEst=[-2.0, 5.5, 0.0], aziEst=[-12.0, 31.0, 0.0], eleEst=[nan, nan, nan])
    r = g(est, _params())
    assert _eq(r.rngRMSE, [0.25, 0.5, nan]) and _eq(r.velRMSE, [1.0, 0.5, nan]) and _eq(r.aziRMSE, [2.0, 1.0, nan]) and _eq(r.eleRMSE, [nan] * 3)
    # exactly one resolution cell away: no match (strict <); just inside: a match
    r = g(SimpleNamespace(rngEst=[101.0, 99.0, 100.9375], velEst=[0.0] * 3, aziEst=[0.0] * 3), _params())
    assert _eq(r.rngRMSE, [nan, nan, 0.9375]) and _eq(r.velRMSE, [nan, nan, 5.0]) and _eq(r.aziRMSE, [nan, nan, 30.0])
    # both truths within the cell: the first in the truth list wins, not the nearer
    r = g(SimpleNamespace(rngEst=[135.0], velEst=[0.0], aziEst=[0.0]), _params(r_res=50.0))
    assert _eq(r.rngRMSE, [35.0]) and _eq(r.velRMSE, [5.0]) and _eq(r.aziRMSE, [30.0])
    # longer velocity / azimuth lists are read at the range list's indices only
    r = g(dict(rngEst=[100.0], velEst=[5.0, 9.0], aziEst=[30.0, 9.0, 9.0], eleEst=[]), _params())
    assert _eq(r.rngRMSE, [0.0]) and _eq(r.velRMSE, [0.0]) and _eq(r.aziRMSE, [0.0]) and r.rngRMSE.shape == (1,)


def test_getRMSE_upa_empty_short_and_target_list():
    g = load_pkg().sensing.postProcessing.getRMSE
    nan = math.nan
    est = SimpleNamespace(rngEst=[100.5, 300.0], velEst=[4.0, 0.0], aziEst=[33.0, 0.0], eleEst=[2.5, 0.0])
    r = g(est, _params("upa"))
    assert _eq(r.eleRMSE, [0.5, nan]) and _eq(r.aziRMSE, [3.0, nan]) and _eq(r.rngRMSE, [0.5, nan]) and _eq(r.velRMSE, [1.0, nan])
    assert _eq(g(est, _params("ula")).eleRMSE, [nan, nan])
    empty = g(SimpleNamespace(rngEst=[], velEst=[], aziEst=[]), _params())
    assert isinstance(empty, float) and math.isnan(empty)
    for bad in (dict(rngEst=[100.0, 140.0], velEst=[5.0], aziEst=[30.0, -10.0]), dict(rngEst=[100.0, 140.0], velEst=[5.0, -3.0], aziEst=[30.0])):
        with pytest.raises(ValueError):
            g(SimpleNamespace(**bad), _params())
    with pytest.raises(ValueError):
        g(SimpleNamespace(rngEst=[100.0, 140.0], velEst=[5.0, -3.0], aziEst=[30.0, -10.0], eleEst=[2.0]), _params("upa"))
    tl = {"rng": np.array([140.5, 100.0]), "vel": np.array([-3.5, 5.0]), "azi": np.array([-10.0, 28.0]), "power": np.array([2.0, 1.0]), "n_total": 2}
    r = g(tl, _params())
    assert _eq(r.rngRMSE, [0.5, 0.0]) and _eq(r.velRMSE, [0.5, 0.0]) and _eq(r.aziRMSE, [0.0, 2.0]) and _eq(r.eleRMSE, [nan, nan])
    # with the truth list of sensing.radarParams itself
    import oracle as O
    pkg = load_pkg()
    cell = O.default_cell_params(n_ants=4, target_pos=((100.0, 20.0, 1.5), (60.0, -30.0, 1.5)), velocity=(7.0, -2.0))
    rp = pkg.sensing.radarParams(cell, SimpleNamespace(NRBsDL=24, SubcarrierSpacing=30), O.nr_ofdm_info(24, 30))
    t = rp.targetRealPos
    r = g({"rng": [t[1]["Range"] + 0.25 * rp.rRes, t[0]["Range"]], "vel": [t[1]["Velocity"], t[0]["Velocity"] - 1.0], "azi": [t[1]["Azimuth"] + 2.0, t[0]["Azimuth"]]}, rp)
    assert np.allclose(r.rngRMSE, [0.25 * rp.rRes, 0.0], atol=1e-9) and np.allclose(r.velRMSE, [0.0, 1.0], atol=1e-12) and np.allclose(r.aziRMSE, [2.0, 0.0], atol=1e-12)
