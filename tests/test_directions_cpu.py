"""isac_resolve_directions (project-defined, include/isac_directions.h) without a GPU: the restatement against the truth on every scene tests/test_gpu_directions.py runs,
the conditioning of those scenes (one local maximum per box), degenerate snapshots, the end-to-end scenes on the oracle, the Python wrapper's row expansion on a stub
and the binding's prototype line.  The device library is not asked for anything but its symbol table."""
from __future__ import annotations

import os
import re
from importlib import import_module

import numpy as np
import pytest

from conftest import ROOT, load_pkg

import _directions_restatement as R

SINGLE_TOL = 1e-9      # lobes: a noise-free single source
FLOOR = 1e-12          # lobes: what the restatement's maximiser is asked to reach; no bound below it


@pytest.mark.parametrize("name", list(R.SINGLE))
def test_single_source(name):
    """A noise-free single source is recovered to 1e-9 of a lobe (amplitude: 1e-9 relative), with nothing left: residual below 1e-20 of ||x||^2 / A; every box the
    maximiser met held exactly one local maximum."""
    s, o = R.scene(name), R.reference(name)
    assert o.boxes_ok and (o.status == 0).all() and (o.n_found == 1).all() and (o.n_src == 1).all()
    for i in range(s.n):
        e_dir, e_amp = R.truth_error(s, o, i)
        print(f"{name}[{i}]: direction {e_dir:.3e} lobes, amplitude {e_amp:.3e} relative, residual {o.residual[i]:.3e}")
        assert e_dir <= SINGLE_TOL and e_amp <= SINGLE_TOL
        assert o.residual[i] <= 1e-20 * (np.abs(s.x[:, i]) ** 2).sum() / s.A


@pytest.mark.parametrize("name", list(R.MULTI))
def test_two_and_three_sources(name):
    """The restatement's error against the truth at cycles = 16, every source of every entry, strongest first.  Measured (lobes): ula16_two 8.9e-15, ula64_two 0, ula256_two 0,
    ula16_three 2.2e-16, upa2x8_two 4.4e-16, upa8x2_two 1.1e-16, upa4x4_three 2.1e-9 (sources 1.5 lobes apart on the circle of a 4-element axis: RELAX converges
    slowly there), upa16x16_two 2.2e-16 -- all but one at the rounding of float64; R.MEASURED_LOBES keeps them and the bound is 10 x that, never below the 1e-12 of the restatement's maximiser.
    Every box the maximiser met -- greedy and all RELAX cycles -- held exactly one local maximum."""
    s, o = R.scene(name), R.reference(name)
    assert o.boxes_ok and (o.status == 0).all() and (o.n_found == s.K).all() and (o.n_src == s.K).all()
    worst = 0.0
    for i in range(s.n):
        e_dir, e_amp = R.truth_error(s, o, i)
        worst = max(worst, e_dir)
        print(f"{name}[{i}]: direction {e_dir:.3e} lobes, amplitude {e_amp:.3e} relative, residual {o.residual[i]:.3e}")
        assert (np.diff(o.power[:, i]) <= 0).all()                         # strongest first
    print(f"{name}: worst {worst:.3e} lobes against the recorded {R.MEASURED_LOBES[name]:.1e}")
    assert worst <= max(10.0 * R.MEASURED_LOBES[name], FLOOR)


def test_one_source_of_two_is_biased():
    """max_sources = 1 on a two-source snapshot: the one direction is off the stronger source by far more than the two-source fit -- what the RELAX cycles remove."""
    s = R.scene("ula16_two")
    one, two = R.reference("ula16_two", 1), R.reference("ula16_two")
    for i in range(s.n):
        bias = R.lobes(s.geom, one.dir_u[0, i] - s.truth[i][0][0])
        print(f"entry {i}: one source {bias:.3e} lobes off, two sources {R.truth_error(s, two, i)[0]:.3e}")
        assert one.n_found[i] == 1 and bias >= 1e-4


def test_degenerate_snapshots():
    """An all-zero and a NaN column: status 1, nothing found, NaN slots; their neighbours' results are those of a run without them."""
    s = R.scene("ula16_two")
    x = np.zeros((16, 4), dtype=np.complex128)
    x[:, 1], x[:, 3] = s.x[:, 0], s.x[:, 1]
    x[5, 2] = np.nan
    o, ref = R.resolve(x, None, 2), R.reference("ula16_two")
    assert o.status.tolist() == [1, 0, 1, 0] and o.n_found.tolist() == [0, 2, 0, 2] and o.n_src.tolist() == [0, 2, 0, 2]
    assert np.isnan(o.dir_u[:, [0, 2]]).all() and np.isnan(o.power[:, [0, 2]]).all() and not o.amp[:, [0, 2]].any()
    assert o.residual[0] == 0.0 and np.isnan(o.residual[2])
    assert o.dir_u[:, [1, 3]].tobytes() == ref.dir_u[:, :2].tobytes() and o.amp[:, [1, 3]].tobytes() == ref.amp[:, :2].tobytes()


def test_floors():
    """min_power above the weaker source: n_src = 1, both still written."""
    s = R.scene("ula16_two")
    o = R.resolve(s.x[:, :1], None, 2, min_power=0.1)
    assert o.n_found.tolist() == [2] and o.n_src.tolist() == [1] and not np.isnan(o.dir_u).any()


def test_end_to_end_on_the_oracle():
    """Two targets in one range-Doppler cell: the list's restatement holds ONE entry for the cell, with one integer azimuth; the restatement on its snapshot gives two
    sources, each within 0.1 degrees (in sind) of a target.  One target at 10.4 degrees: the resolved direction is closer to it than the list's grid azimuth."""
    p = R.oracle_e2e("pair")
    t = p.list
    cell = np.flatnonzero((t.row == t.row[0]) & (t.col == t.col[0]))
    assert cell.size == 1 and float(t.azi[0]).is_integer()
    err = [float(R.u_distance(p.ref.dir_u[k, 0], p.truth_u).min()) for k in range(2)]
    near = [int(R.u_distance(p.ref.dir_u[k, 0], p.truth_u).argmin()) for k in range(2)]
    print(f"pair: list azi {t.azi.tolist()}, resolved dir_u {p.ref.dir_u[:, 0].tolist()}, truth {p.truth_u.tolist()}, errors {err}")
    assert p.ref.n_src[0] == 2 and sorted(near) == [0, 1] and max(err) <= np.sin(np.radians(0.1))
    q = R.oracle_e2e("single")
    fine = float(R.u_distance(q.ref.dir_u[0, 0], q.truth_u[0]))
    grid = float(R.u_distance(np.sin(np.radians(q.list.azi[0])), q.truth_u[0]))
    print(f"single: list azi {q.list.azi[0]}, grid error {grid:.3e}, resolved error {fine:.3e} in sind")
    assert q.list.row.size >= 1 and fine < grid


def test_wrapper_rows_and_twin():
    """sensing.estimation.resolveDirections.expand_rows on a stub of the raw outputs: one row per accepted source in entry order then source order, the entry's fields
    copied, the twin mapping on the host, dir_u / dir_v unchanged by it."""
    import __graft_entry__ as g
    g.build()
    mod = import_module(load_pkg().__name__ + ".sensing.estimation.resolveDirections")
    nan = np.nan
    raw = dict(status=np.array([0, 1, 0], dtype=np.int32), n_found=np.array([2, 0, 2], dtype=np.int32), n_src=np.array([2, 0, 1], dtype=np.int32),
               residual=np.array([0.1, 0.0, 0.3]), azi=np.array([[10.5, nan, -20.25], [-95.0, nan, 40.0]]), ele=np.array([[30.0, nan, 5.0], [60.0, nan, 7.0]]),
               dir_u=np.array([[0.1, nan, 0.3], [0.2, nan, 0.4]]), dir_v=np.array([[0.5, nan, 0.7], [0.6, nan, 0.8]]), power=np.array([[4.0, nan, 9.0], [1.0, nan, 0.01]]),
               amp=np.array([[2.0, 0, 3j], [1j, 0, 0.1]]))
    tl = dict(rng=np.array([10.0, 20.0, 30.0]), vel=np.array([1.0, 2.0, 3.0]), row=np.array([5, 6, 7]), col=np.array([8, 9, 10]), snapshots=None)
    d = mod.expand_rows(raw, tl, upa=False)
    assert d["entry"].tolist() == [0, 0, 2] and d["src"].tolist() == [0, 1, 0]
    assert d["azi"].tolist() == [10.5, -95.0, -20.25] and "ele" not in d and np.isnan(d["dir_v"]).all()
    assert d["dir_u"].tolist() == [0.1, 0.2, 0.3] and d["power"].tolist() == [4.0, 1.0, 9.0] and d["amp"].tolist() == [2.0, 1j, 3j]
    assert d["rng"].tolist() == [10.0, 10.0, 30.0] and d["vel"].tolist() == [1.0, 1.0, 3.0] and d["row"].tolist() == [5, 5, 7] and d["col"].tolist() == [8, 8, 10]
    assert d["n_src"].tolist() == [2, 0, 1] and d["n_found"].tolist() == [2, 0, 2] and d["status"].tolist() == [0, 1, 0] and d["residual"].tolist() == [0.1, 0.0, 0.3]
    tw = mod.expand_rows(raw, tl, upa=False, twin=True)
    assert tw["azi"].tolist() == [169.5, -85.0, -159.75] and tw["dir_u"].tolist() == d["dir_u"].tolist()
    up = mod.expand_rows(raw, np.zeros((4, 3)), upa=True)
    assert up["ele"].tolist() == [30.0, 60.0, 5.0] and up["dir_v"].tolist() == [0.5, 0.6, 0.7] and "rng" not in up
    ut = mod.expand_rows(raw, None, upa=True, twin=True)
    assert ut["ele"].tolist() == [-30.0, -60.0, -5.0] and ut["azi"].tolist() == [-169.5, 85.0, 159.75] and ut["dir_v"].tolist() == up["dir_v"].tolist()
    u0 =np.sin(np.radians(up["ele"])) * np.cos(np.radians(up["azi"]))
    u1 = np.sin(np.radians(ut["ele"])) * np.cos(np.radians(ut["azi"]))   # a twin is the same direction
    assert np.abs(u0 - u1).max() < 1e-15
    empty = mod.expand_rows({k: v[..., :0] for k, v in raw.items()}, dict(rng=np.zeros(0)), upa=False)
    assert empty["azi"].size == 0 and empty["entry"].size == 0 and empty["rng"].size == 0


def test_binding_has_the_prototype_and_the_abi_is_unchanged():
    """include/isac_directions.h is additive under ABI 8: no new struct, no new isac_abi_sizeof selector; the header carries the defaults, and its one function refuses a
    NULL context.  (Its prototype line is compared with the header by tests/test_abi_cpu.py, row "isac_directions.h".)"""
    import __graft_entry__ as g
    g.build()
    L = load_pkg()._lib
    hdr = open(os.path.join(ROOT, "include", "isac_directions.h")).read()
    plain = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    assert "typedef" not in plain and "ISAC_SIZEOF" not in plain
    for macro, want in (("MAX_SOURCES", 8), ("CYCLES", 16), ("MIN_RATIO", 0.01)):
        assert float(re.search(rf"#define ISAC_DIR_{macro} ([0-9.]+)", plain).group(1)) == want
    assert L.ISAC_DIR_MAX_SOURCES == 8 == R.MAX_SOURCES
    lib = L.load()                                                             # (needs no GPU)
    assert lib.isac_abi_version() == 8 == L.ISAC_ABI_VERSION and lib.isac_abi_sizeof(13) == -1
    fn = lib.isac_resolve_directions
    assert fn(None, None, None, 4, 0, 1, 16, 0.01, 0.0, None, None, None, None, None, None, None, None, None, None) == 1   # refused before anything touches a device: no context
    assert callable(load_pkg().sensing.estimation.resolveDirections)
