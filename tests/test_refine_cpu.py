"""isac_fft2d_refine_targets (project-defined, include/isac_refine.h) without a GPU: the conditioning of every scene tests/test_gpu_refine.py runs, on the oracle alone;
the restatement's handling of degenerate rows; the binding's prototype line.  The device library is not asked for anything but its symbol table."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_pkg

import _refine_restatement as R

MARGIN = 1e-6


@pytest.mark.parametrize("name", list(R.SCENES))
def test_scene_conditioning(name):
    """Every margin of every decision of steps 2, 4 and 5 is at least 1e-6 (step 2: relative; step 4: in units of 1/L; step 5: in log2 of the ratio to the threshold), and
    the refined velocity of every entry that is not flagged a sidelobe is strictly closer to the scene's true velocity than the grid velocity."""
    s = R.oracle_scene(name)
    r = s.ref
    print(f"{name}: L {s.L}, nFFT {s.n_fft}; rows {s.row.tolist()} cols {s.col.tolist()} -> parent {r.parent.tolist()} sidelobe_of {r.sidelobe_of.tolist()}; refined bins "
          f"{(r.nu * s.n_fft).round(4).tolist()}; smallest margins: step 2 {r.m2.min():.3e}, step 4 {min(r.m4, default=np.inf):.3e}, step 5 {min(r.m5, default=np.inf):.3e}")
    assert s.row.size >= R.MIN_ENTRIES.get(name, 2) and (r.status == 0).all()
    assert r.m2.min() >= MARGIN and min(r.m4, default=np.inf) >= MARGIN and min(r.m5, default=np.inf) >= MARGIN
    checked = 0
    for i in np.flatnonzero((r.parent == np.arange(s.row.size)) & (r.sidelobe_of < 0)):
        truth = R.true_velocity(s, i)
        assert truth is not None
        print(f"  entry {i}: truth {truth / s.rp.vRes:.4f} bins, grid {s.grid_vel[i] / s.rp.vRes:.0f}, refined {r.vel[i] / s.rp.vRes:.4f}")
        assert abs(r.vel[i] - truth) < abs(s.grid_vel[i] - truth)
        checked += 1
    assert checked >= R.MIN_ENTRIES.get(name, 2)


@pytest.mark.parametrize("name", ["split273", "split273_a8"])
def test_split_scene_six_entries_become_two_targets(name):
    """6 listed entries -> 5 kept, exactly 2 of them unflagged: the representative of the merged pair (the two lobes of the stronger target's tone, merged at distance
    zero against the tolerance 0.5) and the second target."""
    s = R.oracle_scene(name)
    r = s.ref
    assert s.row.size == 6 and r.n_kept == 5
    merged = np.flatnonzero(r.parent != np.arange(6))
    assert merged.size == 1
    i, k = int(merged[0]), int(r.parent[merged[0]])
    assert {(int(s.row[i]), int(s.col[i])), (int(s.row[k]), int(s.col[k]))} == set(R.SPLIT_LOBES)
    assert abs(r.nu[i] - r.nu[k]) * s.L < 1e-9
    kept = np.flatnonzero(r.parent == np.arange(6))
    clean = kept[r.sidelobe_of[kept] < 0]
    assert clean.size == 2 and clean[0] == k
    truths = {R.true_velocity(s, j) for j in clean}
    assert truths == {float(t["Velocity"]) for t in s.rp.targetRealPos}          # one entry per physical target
    assert all(r.sidelobe_of[j] in clean for j in kept if r.sidelobe_of[j] >= 0)  # every flag points at a physical target
    off = R.refine(s.rows_of(s.row), s.row, s.col, s.n_fft, float(s.rp.vRes), merge_tol=0.0, sidelobe_margin=0.0)
    assert off.n_kept == 6 and (off.sidelobe_of == -1).all() and off.nu.tobytes() == r.nu.tobytes()   # both steps off: every entry kept, none flagged, the values as before


def test_degenerate_rows_take_no_part():
    """An all-zero row and a row holding a NaN: status 1, nu = nu0, the grid velocity, parent = itself, never a representative, never flagged or flagging."""
    s = R.oracle_scene("split24")
    good = s.rows_of(s.row[:1])[0]
    zero, nan = np.zeros_like(good), good.copy()
    nan[3, 1] = np.nan
    Y = np.stack([zero, good, nan, good, zero])
    row, col = np.full(5, s.row[0]), np.full(5, s.col[0])
    r = R.refine(Y, row, col, s.n_fft, float(s.rp.vRes))
    assert r.status.tolist() == [1, 0, 1, 0, 1]
    assert r.parent.tolist() == [0, 1, 2, 1, 4] and r.sidelobe_of.tolist() == [-1] * 5 and r.n_kept == 4
    nu0 = (s.col[0] - s.n_fft // 2 - 1) / s.n_fft
    assert r.nu[0] == r.nu[2] == r.nu[4] == nu0 and r.vel[0] == r.vel[2] == s.grid_vel[0]
    assert r.power[0] == 0.0 and np.isnan(r.power[2]) and not r.snapshots[:, 0].any() and np.isnan(r.snapshots[:, 2]).any()
    assert r.nu[1] == s.ref.nu[0] and r.power[1] == s.ref.power[0]


def test_probe_plan():
    """W = max(1/L, 1/nFFT), M = ceil(8 L W): 17 probes over +-1/L where nFFT >= L."""
    assert R.probe_plan(56, 256) == (1 / 56, 8) and R.probe_plan(28, 64) == (1 / 28, 8) and R.probe_plan(28, 16) == (1 / 16, 14) and R.probe_plan(64, 64) == (1 / 64, 8)


def test_binding_has_the_prototype_and_the_abi_is_unchanged():
    """include/isac_refine.h is additive under ABI 8: no new struct, no new isac_abi_sizeof selector; the header carries the defaults and says what is out of scope, and
    its one function refuses a NULL context.  (Its prototype line is compared with the header by tests/test_abi_cpu.py, row "isac_refine.h".)"""
    import __graft_entry__ as g
    g.build()
    L = load_pkg()._lib
    hdr = open(os.path.join(ROOT, "include", "isac_refine.h")).read()
    plain = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    assert "typedef" not in plain and "ISAC_SIZEOF" not in plain
    for macro, want in (("MERGE_TOL", 0.5), ("MERGE_ROWS", 1), ("SIDELOBE_MARGIN", 2.0)):
        assert float(re.search(rf"#define ISAC_REFINE_{macro} ([0-9.]+)", plain).group(1)) == want
    for word in ("OUT OF SCOPE", "off-grid range", "off-grid direction", "range sidelobes", "MEX"):
        assert word in hdr
    lib = L.load()                                                             # (needs no GPU)
    assert lib.isac_abi_version() == 8 == L.ISAC_ABI_VERSION and lib.isac_abi_sizeof(13) == -1
    fn = lib.isac_fft2d_refine_targets
    assert fn(None, None, None, 0, 0.5, 1, 2.0, None, None, None, None, None, None, None, None, None, None) == 1   # refused before anything touches a device: no context
    est = load_pkg().sensing.estimation
    assert callable(est.refineTargets)
