"""The per-target list of fft2D (isac_fft2d_get_targets; project-defined, include/isac_targets.h) without a GPU: the NumPy restatement on hand-made maps and known snapshots,
the binding's prototype line, and the conditioning of every scene tests/test_gpu_target_list.py uses -- on the oracle chain each scene must have targets where the
true targets are, and every decision the list rests on must clear the project's 1e-9 guard band, so that the GPU tests leave out no case."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest

import oracle as O
from conftest import load_pkg

import _target_list_restatement as R

RECT7 = (2, 6, 2, 6)          # CUT zone of a 7 x 7 map with a one-cell halo


def _toy(peaks, base=1.0):
    S = np.full((7, 7), base)
    for (r, c), v in peaks.items():
        S[r - 1, c - 1] = v
    return S[:, :, None] * np.array([0.25, 0.75])[None, None, :]      # two antennas; the halves add back exactly


def _det(*cells):
    return np.array(cells, dtype=np.int64).T.reshape(2, -1)


def test_two_maxima_on_a_7x7_map():
    P = _toy({(3, 3): 9.0, (5, 5): 4.0, (3, 4): 2.0})
    t = R.target_cells(P, [_det((3, 3), (5, 5), (3, 4)), _det((3, 3))], 1, 1, RECT7, 7)
    assert t.row.tolist() == [3, 5] and t.col.tolist() == [3, 5] and t.hits.tolist() == [2, 1] and t.power.tolist() == [9.0, 4.0]
    assert np.allclose(t.margin1, [(9.0 - 2.0) / 9.0, (4.0 - 1.0) / 4.0])


def test_a_plateau_gives_no_target_and_nan_is_never_one():
    P = _toy({(3, 3): 5.0, (3, 4): 5.0})
    assert R.target_cells(P, [_det((3, 3), (3, 4))], 1, 1, RECT7, 7).row.size == 0
    P = _toy({(4, 4): np.nan, (2, 2): 3.0})
    t = R.target_cells(P, [_det((4, 4), (2, 2), (3, 3))], 1, 1, RECT7, 7)
    assert t.row.tolist() == [2] and t.col.tolist() == [2]                    # (3, 3) has a NaN neighbour, (4, 4) is NaN


def test_a_maximum_without_a_detection_gives_no_target():
    P = _toy({(3, 3): 9.0, (5, 5): 4.0})
    t = R.target_cells(P, [_det((5, 5))], 1, 1, RECT7, 7)
    assert t.row.tolist() == [5] and t.hits.tolist() == [1]


def test_an_exact_tie_is_ordered_by_column_major_index():
    P = _toy({(6, 2): 4.0, (2, 4): 4.0, (4, 6): 7.0, (2, 2): 4.0})
    t = R.target_cells(P, [_det((6, 2), (2, 4), (4, 6), (2, 2))], 1, 1, RECT7, 7)
    assert list(zip(t.row.tolist(), t.col.tolist())) == [(4, 6), (2, 2), (6, 2), (2, 4)]   # ties: r + 7 (c - 1) = 2, 6, 23


def test_a_window_without_halo_is_refused():
    with pytest.raises(ValueError):
        R.target_cells(_toy({}), [], 1, 1, (1, 7, 2, 6), 7)


@pytest.mark.parametrize("n_ants", [4, 8, 16])
def test_known_snapshots_kat5(n_ants):
    """x = a(phi0) gives phi0 for integer phi0 in (0, 90) and -180 - phi0 for phi0 in (-90, 0): the mirror twin with the lower scan index (SURVEY KAT-5)."""
    rp = R.make("a4_24prb_generic").rp
    m = np.arange(n_ants)
    phis = np.array([1, 17, 30, 45, 60, 89, -1, -17, -30, -45, -60, -89], dtype=np.float64)
    x = np.stack([np.exp(-2j * np.pi * m * 0.5 * float(O.sind(p))) for p in phis], axis=1)
    bins, azi, margin2, B = R.bartlett(x, rp)
    want = np.where(phis > 0, phis, -180.0 - phis)
    assert np.array_equal(azi, want)
    twin = (np.where(want > 0, 180.0 - want, -180.0 - want) + 180.0).astype(int)   # scan index of the mirror angle
    assert all(B[b, t] == B[tw, t] for t, (b, tw) in enumerate(zip(bins, twin)))   # mirror twins are bitwise equal
    assert (margin2 > 0).all()


def test_binding_has_the_prototype_and_the_abi_version_is_unchanged():
    """The entry point is additive under ABI 8: it is declared in include/isac_targets.h, and the binding carries its struct as selector 11 of ABI_STRUCTS.  (Its
    prototype line is compared with the header by tests/test_abi_cpu.py, row "isac_targets.h".)"""
    import os
    import re
    import __graft_entry__ as g
    from conftest import ROOT
    g.build()
    L = load_pkg()._lib
    assert L.ISAC_ABI_VERSION == 8
    hdr = open(os.path.join(ROOT, "include", "isac_targets.h")).read()
    sel = int(re.search(r"#define ISAC_SIZEOF_TARGET_LIST (\d+)", hdr).group(1))
    assert sel == 11 and L.ABI_STRUCTS[sel] == ("isac_target_list", L.TargetList)
    assert int(re.search(r"#define ISAC_MAX_TARGETS (\d+)", hdr).group(1)) == L.ISAC_MAX_TARGETS == 1024
    assert ctypes.sizeof(L.TargetList) == 8 + 1024 * (3 * 4 + 4 * 8)
    lib = L.load()                                                             # (needs no GPU) load() checked the struct size
    assert lib.isac_abi_sizeof(sel) == ctypes.sizeof(L.TargetList) and lib.isac_abi_version() == 8


@pytest.mark.parametrize("name", list(R.SCENES))
def test_scene_conditioning(name):
    """Oracle chain -> restatement for every scene of the GPU tests: at least one target, the strongest Q entries at the true targets' range rows (SURVEY KAT-3), and
    EVERY target with both margins (and every detected near-miss) at least 1e-9 relative away from the other decision."""
    sc = R.make(name)
    t = R.oracle_targets(name)
    q = len(sc.rp.range)
    print(f"{name}: {t.row.size} targets, rows {t.row[:6].tolist()} cols {t.col[:6].tolist()} hits {t.hits[:6].tolist()} azi {t.azi[:6].tolist()}; "
          f"min margin1 {t.margin1.min():.3e}, min margin2 {t.margin2.min():.3e}, near miss {t.near_miss:.3e}; aziEst {t.est.aziEst.tolist()}")
    assert t.row.size >= 1
    assert t.row.size >= q                                                     # sidelobes that CFAR detects are local maxima too
    want_rows = sorted(math.ceil(2.0 * r * sc.rp.fs / O.LIGHTSPEED) + 1 for r in sc.rp.range)
    assert sorted(t.row[:q].tolist()) == want_rows
    assert (t.margin1 >= R.GUARD_BAND).all() and (t.margin2 >= R.GUARD_BAND).all()
    assert t.near_miss >= R.GUARD_BAND
    assert np.array_equal(t.rng, (t.row - 1) * sc.rp.rRes)


def test_single_target_bartlett_is_not_music():
    """One target, 8 elements, on the oracle: the strongest entry's Bartlett azimuth differs from fft2D's aziEst -- so the GPU tests make no such comparison.  Why: the
    echo of transmit element t arrives at receive element a with steering a[t] a[a] (basicRadarChannel.m:51, (e*a)*a.'), and rdm(:,:,a) matched-filters receive plane a
    against ITS OWN transmit plane (fft2D.m:37), which keeps the path t = a: the snapshot carries the TWO-WAY phase, x[m] ~ a[m]^2 = exp(2j pi m 2f).  MUSIC works on Ra
    of the raw grid, one-way, and conjugated (fft2D.m:106-107 reshapes with a conjugate transpose): exp(-2j pi m f).  Against the scan vector exp(-2j pi m 0.5 sind(phi))
    the first peaks where 0.5 sind(phi) = -2f, the second where 0.5 sind(phi) = f (both modulo 1): sind(azi) = -2 sind(aziEst) up to the 1-degree grid."""
    t = R.oracle_targets("a8_single")
    azi, est = float(t.azi[0]), t.est.aziEst
    s_b, s_m = float(O.sind(azi)), float(O.sind(est[0]))
    print(f"a8_single: Bartlett azi {azi}, aziEst {est.tolist()}; sind {s_b:.4f} against -2 x {s_m:.4f}; margins {t.margin1.min():.3e} {t.margin2.min():.3e}")
    assert azi not in est.tolist()
    wrapped = (s_b + 2.0 * s_m + 1.0) % 2.0 - 1.0                              # 0.5 sind is defined modulo 1, so sind modulo 2
    assert abs(wrapped) <= 3.0 * np.pi / 360.0                                 # half a 1-degree step moves sind by at most pi/360: once for the Bartlett bin, twice for 2 sind(aziEst)
    assert (t.margin1 >= R.GUARD_BAND).all() and (t.margin2 >= R.GUARD_BAND).all()
