"""UPA direction finding without a GPU: the ABI of ISAC_OPT_UPA_DOA / isac_get_angular_spectrum2d / isac_find2d_peaks, and known-answer tests of
the restatement (tests/_upa_restatement.py) the GPU tests compare against -- the mirror-twin tie, the column normalisation quirk, find2DPeaks' rules."""
from __future__ import annotations

import ctypes as C
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import _upa_restatement as R
from conftest import load_pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rp():
    return SimpleNamespace(azimuthScanScale=360, azimuthScanGranularity=1, elevationScanScale=180, elevationScanGranularity=1)


def test_abi_version_and_symbols():
    pkg = load_pkg()
    lib = pkg._lib.load()
    assert lib.isac_abi_version() == 8 == pkg._lib.ISAC_ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "isac.h")).read()
    assert re.search(r"#define ISAC_ABI_VERSION 8\b", hdr)
    assert re.search(r"ISAC_OPT_UPA_DOA\s*=\s*4", hdr)
    for name in ("isac_get_angular_spectrum2d", "isac_find2d_peaks"):
        assert name in pkg._lib.HEADER_PROTOTYPES["isac.h"] and name + "(" in hdr
        getattr(lib, name)


def test_grid_defaults():
    ele, azi = R.grid(_rp())
    assert ele.size == 181 and azi.size == 361 and ele[0] == -90 and azi[0] == -180 and ele[-1] == 90 and azi[-1] == 180


@pytest.mark.parametrize("n_v,n_h", [(4, 4), (8, 8)])
@pytest.mark.parametrize("ele0,azi0", [(20.0, 35.0), (-30.0, -60.0), (45.0, 120.0)])
def test_music_top_peaks_are_direction_and_twin(n_v, n_h, ele0, azi0):
    """Ra = a0 a0' + sigma^2 I with the scan's own steering at a grid direction: MUSIC's two highest peaks are exactly that direction and its
    mirror twin (ph -+ 180, -th), tied, the one with the smaller azimuth first."""
    rp = _rp()
    ph = R.steering_phases(n_v, n_h, np.array([ele0]), np.array([azi0]))[0]
    a0 = np.exp(1j * ph)
    ra = np.outer(a0, a0.conj()) + 0.01 * np.eye(n_v * n_h)
    L, azi, ele, pdb = R.doa(0, ra, n_v, n_h, rp, num_dets=2)
    twin = (-ele0, azi0 - 180.0 if azi0 >= 0 else azi0 + 180.0)
    got = list(zip(ele, azi))
    want = sorted([(ele0, azi0), twin], key=lambda t: t[1])
    assert got == want
    e0, a0i = int(ele0 + 90), int(azi0 + 180)
    assert pdb[e0, a0i] == pdb[180 - e0, R.twin_columns(361)[a0i]]


@pytest.mark.parametrize("method", [0, 1, 2])
def test_every_column_minimum_is_zero_db(method):
    rng = np.random.default_rng(3)
    n_v, n_h = 4, 4
    x = rng.standard_normal((16, 40)) + 1j * rng.standard_normal((16, 40))
    ra = x @ x.conj().T / 40
    pdb, _ = R.spectrum_db(method, ra, n_v, n_h, _rp(), num_dets=2)
    assert pdb.shape == (181, 361)
    assert np.all(pdb.min(axis=0) == 0.0) and np.all(pdb >= 0.0)


def test_twins_tie_on_the_whole_map():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((16, 30)) + 1j * rng.standard_normal((16, 30))
    pdb, _ = R.spectrum_db(1, x @ x.conj().T / 30, 4, 4, _rp())
    assert np.array_equal(pdb, pdb[::-1, R.twin_columns(361)])


def test_find2d_peaks_rules():
    m = np.zeros((5, 6))
    m[0, 2] = 9.0                  # border maximum: never a peak
    m[4, 5] = 9.0
    m[2, 2] = 3.0                  # interior strict maximum
    m[2, 4] = 3.0                  # equal value, larger column-major index
    m[1, 1] = 1.0                  # interior, but its neighbour (2, 2) is higher
    ele, azi = R.find_2d_peaks(m, 5)
    assert list(ele) == [3, 3] and list(azi) == [3, 5]              # fewer candidates than L; tie in column-major order
    ele, azi = R.find_2d_peaks(m, 1)
    assert list(ele) == [3] and list(azi) == [3]
    p = np.zeros((6, 6))
    p[2:4, 2:4] = 4.0              # plateau: no peak
    assert R.find_2d_peaks(p, 3)[0].size == 0
    q = np.zeros((5, 5))
    q[1, 1], q[3, 3] = 2.0, 2.0    # equal values: the smaller column-major index first
    q[1, 3] = 5.0
    ele, azi = R.find_2d_peaks(q, 3)
    assert list(zip(ele, azi)) == [(2, 4), (2, 2), (4, 4)]
    with pytest.raises(ValueError):
        R.find_2d_peaks(q, 0)
