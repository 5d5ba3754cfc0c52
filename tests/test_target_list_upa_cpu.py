"""The UPA per-target list (isac_fft2d_get_targets_upa; project-defined, include/isac_targets_upa.h) without a GPU: the conditioning of every scene
tests/test_gpu_target_list_upa.py uses, the restatement of step 4 against a brute-force evaluation, the binding's prototype line, and getRMSE on a list that carries
elevations."""
from __future__ import annotations

import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ROOT, load_pkg

import _abi_header as H
import _target_list_upa_restatement as R
import _upa_restatement as U


@pytest.mark.parametrize("name", list(R.SCENES))
def test_scene_conditioning(name):
    """Oracle stages -> restatement for every scene of the GPU tests: at least one target, and EVERY decision of every target (margin 1, margin 2, every detected near-miss)
    at least 1e-9 relative away from the other one -- the GPU tests then leave out and skip nothing.  Every target's winner ties with its mirror twin and nothing else."""
    t = R.oracle_targets(name)
    print(f"{name}: {t.row.size} targets, rows {t.row[:6].tolist()} cols {t.col[:6].tolist()} hits {t.hits[:6].tolist()} azi {t.azi[:6].tolist()} ele {t.ele[:6].tolist()}; "
          f"min margin1 {t.margin1.min():.3e}, min margin2 {t.margin2.min():.3e}, near miss {t.near_miss:.3e}, ties {t.ties.tolist()}")
    assert t.row.size >= 1
    assert (t.margin1 >= R.GUARD_BAND).all() and (t.margin2 >= R.GUARD_BAND).all()
    assert t.near_miss >= R.GUARD_BAND
    assert (t.ties == 2).all()
    sc = R.make(name)
    assert all(int(j) == R.lowest_equal(j, sc.nV, sc.nH, sc.rp) for j in t.j)


def _coarse(n_v, n_h):
    return SimpleNamespace(antennaType=SimpleNamespace(kind="upa", nV=n_v, nH=n_h), azimuthScanScale=360, azimuthScanGranularity=15, elevationScanScale=180,
                           elevationScanGranularity=15)


@pytest.mark.parametrize("n_v,n_h", [(2, 4), (4, 2), (4, 4)])
def test_restatement_against_brute_force(n_v, n_h):
    """A 15-degree grid (12 elevations -90 .. 75, 24 azimuths -180 .. 165), x = a_j0: a per-point loop without `unique` and the restatement both return min(j0, twin(j0)),
    the twin of (e, a) being (12 - e, a -+ 12) -- elevation -th, azimuth ph -+ 180; row e = 0 (-90 degrees) has no twin on this grid."""
    rp = _coarse(n_v, n_h)
    ele, azi = U.grid(rp)
    assert ele.size == 12 and azi.size == 24 and ele[0] == -90.0 and azi[0] == -180.0
    ph = U.steering_phases(n_v, n_h, ele, azi)
    for e, a in ((2, 3), (4, 14), (9, 20), (10, 1), (3, 23), (0, 5)):
        j0 = e + 12 * a
        twin = (12 - e) + 12 * (a + 12 if a < 12 else a - 12) if e >= 1 else j0
        if e >= 1:
            assert ph[twin].tobytes() == ph[j0].tobytes()                    # the twins' steering vectors are bitwise equal
        x = np.exp(1j * ph[j0])
        want = min(j0, twin)
        assert R.bartlett2d_brute(x, n_v, n_h, rp) == want
        js, azi_t, ele_t, margin2, ties = R.bartlett2d(x, n_v, n_h, rp)
        assert int(js[0]) == want and azi_t[0] == azi[want // 12] and ele_t[0] == ele[want % 12]
        assert ties[0] == (2 if e >= 1 else 1) and margin2[0] > 0
        assert R.lowest_equal(j0, n_v, n_h, rp) == want


def test_binding_has_the_prototype_and_the_abi_is_unchanged():
    """include/isac_targets_upa.h is additive under ABI 8: no new struct, no new isac_abi_sizeof selector; its one function takes the C types below and refuses a NULL
    context.  (Its prototype line is compared with the header by tests/test_abi_cpu.py, row "isac_targets_upa.h".)"""
    import __graft_entry__ as g
    g.build()
    L = load_pkg()._lib
    hdr = open(os.path.join(ROOT, "include", "isac_targets_upa.h")).read()
    plain = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    assert "typedef" not in plain and "ISAC_SIZEOF" not in plain
    assert [types for _, _, types in H.prototypes("isac_targets_upa.h")] == [["isac_ctx*", "isac_target_list*", "double*", "isac_c64*", "int32_t"]]
    lib = L.load()                                                             # (needs no GPU)
    assert lib.isac_abi_version() == 8 == L.ISAC_ABI_VERSION and lib.isac_abi_sizeof(13) == -1
    assert lib.isac_fft2d_get_targets_upa(None, None, None, None, 0) == 1      # refused before anything touches a device: no context (ISAC_ERR_INVALID_ARG)
    est = load_pkg().sensing.estimation
    assert callable(est.targetListUPA) and est.targetListUPA is not est.targetList


def _params(kind):
    truth = [dict(ID=1, Range=100.0, Velocity=5.0, Elevation=2.0, Azimuth=30.0, snrdB=20.0), dict(ID=2, Range=140.0, Velocity=-3.0, Elevation=-4.0, Azimuth=-10.0, snrdB=10.0)]
    return SimpleNamespace(rRes=1.0, antennaType=SimpleNamespace(kind=kind), targetRealPos=truth)


def _eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b, dtype=np.float64), equal_nan=True)


def test_getRMSE_accepts_a_list_with_elevations():
    g = load_pkg().sensing.postProcessing.getRMSE
    nan = math.nan
    tl = {"rng": np.array([140.5, 100.0, 300.0]), "vel": np.array([-3.5, 5.0, 0.0]), "azi": np.array([-10.0, 28.0, 0.0]), "ele": np.array([-5.0, 2.25, 0.0]),
          "power": np.array([3.0, 2.0, 1.0]), "n_total": 3}
    r = g(tl, _params("upa"))
    assert _eq(r.rngRMSE, [0.5, 0.0, nan]) and _eq(r.velRMSE, [0.5, 0.0, nan]) and _eq(r.aziRMSE, [0.0, 2.0, nan]) and _eq(r.eleRMSE, [1.0, 0.25, nan])
    no_ele = {k: v for k, v in tl.items() if k != "ele"}
    with pytest.raises(ValueError, match="no elevation"):                      # targetList's dict on UPA parameters: as before
        g(no_ele, _params("upa"))
    with pytest.raises(ValueError):                                            # fewer elevations than ranges
        g({**tl, "ele": np.array([1.0])}, _params("upa"))
    # a ULA: today's result, whether or not the dict carries elevations
    for d in (no_ele, tl):
        r = g(d, _params("ula"))
        assert _eq(r.rngRMSE, [0.5, 0.0, nan]) and _eq(r.velRMSE, [0.5, 0.0, nan]) and _eq(r.aziRMSE, [0.0, 2.0, nan]) and _eq(r.eleRMSE, [nan] * 3)
    est = SimpleNamespace(rngEst=[100.5, 300.0], velEst=[4.0, 0.0], aziEst=[33.0, 0.0], eleEst=[2.5, 0.0])
    r = g(est, _params("upa"))
    assert _eq(r.eleRMSE, [0.5, nan]) and _eq(r.aziRMSE, [3.0, nan]) and _eq(r.rngRMSE, [0.5, nan]) and _eq(r.velRMSE, [1.0, nan])
