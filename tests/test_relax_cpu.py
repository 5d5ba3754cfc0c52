"""isac_fft2d_relax_targets (project-defined, include/isac_relax.h) without a GPU: what the joint re-fit recovers on exact tones and on the oracle's chain, the properties
of the rule (cycles = 0 is the cancellation of isac_clean.h, the cluster schedule is the sequential sweep, the residual energy does not rise), the conditioning of every
case tests/test_gpu_relax.py runs, and the binding's prototype line.  The device library is not asked for anything but its symbol table."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_pkg

import _clean_restatement as K
import _relax_restatement as X

MARGIN = 1e-6


@pytest.fixture(scope="module", autouse=True)
def binding():
    """The restatement restates a call of the library: every test here needs the call to exist (built, exported, bound)."""
    import __graft_entry__ as g
    g.build()
    L = load_pkg()._lib
    assert list(L.HEADER_PROTOTYPES["isac_relax.h"]) == ["isac_fft2d_relax_targets"] and hasattr(L.load(), "isac_fft2d_relax_targets")
    return L


@pytest.mark.parametrize("L", [28, 112])
def test_exact_tones_are_recovered(L):
    """Two exact tones on one row, 1.3 / L apart, amplitudes 1 : 0.5, four antennas, no noise.  The sequential estimates (each tone once, the later one still in the data)
    are off by 1e-3 lobes or more on at least one tone (measured: 1.2e-2 and 1.6e-2 at L = 28, 1.2e-2 and 1.5e-2 at L = 112); 16 cycles from there end within 1e-6 lobes of
    the truth on both (measured: 4.5e-13, the width of the last bracket).  One tone alone does not move."""
    nus = np.array([0.011, 0.011 + 1.3 / L])
    rows = X.tone_rows(L, nus, (1.0, 0.5))
    seq = X.sequential(rows, [0, 0], nus, 64)
    r = X.relax(rows, [0, 0], seq, 64, cycles=16, span_rows=0)
    e_seq, e_relax = np.abs(seq - nus) * L, np.abs(r.nu - nus) * L
    print(f"L = {L}: sequential {e_seq.tolist()}, after 16 cycles {e_relax.tolist()} lobes; last step {r.last_step.tolist()}; residual energy {r.energy[0]:.3e} -> {r.energy[-1]:.3e}")
    assert e_seq.max() >= 1e-3
    assert e_relax.max() <= 1e-6 and (r.status == 0).all() and r.decisions.all()
    one = X.tone_rows(L, nus[:1], (1.0,))
    start = X.sequential(one, [0], nus[:1], 64)
    alone = X.relax(one, [0], start, 64, cycles=16, span_rows=0)
    print(f"L = {L}: one tone: shift {alone.shift[0]:.3e}")
    assert alone.shift[0] <= 1e-9 and abs(start[0] - nus[0]) * L <= 1e-9


def test_no_cycle_is_the_cancellation_of_clean():
    """cycles = 0: R is step 8 of isac_clean.h for the same entries in the same order (tests/_clean_restatement.py: replay, long double throughout), to the rounding of
    one fp64 store per pass; the amplitudes are what was subtracted; nu, shift, last_step and status are those of a call that searched nothing."""
    for case in ("pair_cycles0", "three_clusters", "edge_rows"):
        s = X.oracle_rows(X.CASES[case][0])
        row, nu = X.entries(case)
        span = X.CASES[case][2].get("span_rows", X.SPAN_ROWS)
        r = X.run(case, s.rows, cycles=0)
        ref = K.replay(s.rows, s.g, row, nu, span)
        err = float(np.abs(r.residual.astype(np.clongdouble) - ref).max())
        bound = 16 * s.L * 2.0 ** -53 * np.abs(s.rows).max()
        print(f"{case}: residual against the replay {err:.3e} (bound {bound:.3e})")
        assert err <= bound
        assert r.nu.tobytes() == nu.tobytes() and not r.shift.any() and not r.last_step.any() and not r.status.any() and r.decisions.shape == (0, row.size)
    assert X.oracle_relax("pair_cycles0").residual.tobytes() == X.run("pair", X.oracle_rows("a4_L28").rows, cycles=0).residual.tobytes()


@pytest.mark.parametrize("case", ["three_clusters", "sixty_four", "edge_rows", "adjacent_rows"])
def test_cluster_schedule_is_the_sequential_sweep(case):
    """The device's order -- the k-th entry of every cluster side by side -- gives the bytes of the sweep in input order: clusters share no row."""
    s = X.oracle_rows(X.CASES[case][0])
    row, _ = X.entries(case)
    kw = X.CASES[case][2]
    wr = row - s.g.first_row
    cl = X.clusters(wr, s.g.n_rows, kw.get("span_rows", X.SPAN_ROWS))
    served = X.order(wr, s.g.n_rows, kw.get("span_rows", X.SPAN_ROWS), "cluster")
    print(f"{case}: clusters {cl}; served {served}")
    assert sorted(served) == list(range(row.size)) and all(c == sorted(c) for c in cl)
    if case == "three_clusters":
        assert cl == [[0, 3], [1, 4], [2]] and served == [0, 1, 2, 3, 4]
        rev = X.order(wr[::-1], s.g.n_rows, 2, "cluster")                  # the same entries given backwards: [4 1], [3 0], [2] -> positions 0 then 1
        assert rev == [0, 1, 2, 3, 4] and X.clusters(wr[::-1], s.g.n_rows, 2) == [[0, 3], [1, 4], [2]]
    if case == "edge_rows":
        assert cl == [[0, 2], [1]]                                         # span 3: rows 6 and 12 share row 9
    if case in ("sixty_four", "adjacent_rows"):
        assert len(cl) == 1
    seq, dev = X.oracle_relax(case), X.run(case, s.rows, schedule="cluster")
    for k in ("nu", "status", "power", "snapshots", "residual", "decisions", "last_step"):
        assert getattr(seq, k).tobytes() == getattr(dev, k).tobytes(), k
    assert all(a.tobytes() == b.tobytes() for a, b in zip(seq.C, dev.C))


def test_cluster_schedule_reorders_and_still_agrees():
    """Three entries in one cluster and a fourth far away: the device serves them as 0, 3, 1, 2 -- the far entry beside the first -- and gives the bytes of 0, 1, 2, 3."""
    s = X.oracle_rows("a4_L28")
    wr = np.array([X.TARGET_ROW, X.TARGET_ROW, X.TARGET_ROW + 1, X.TARGET_ROW + 9]) - s.g.first_row
    nu = np.array([s.nu[0], s.nu[1], 2.3 / s.L, 1.9 / s.L])
    assert X.clusters(wr, s.g.n_rows, 2) == [[0, 1, 2], [3]] and X.order(wr, s.g.n_rows, 2, "cluster") == [0, 3, 1, 2]
    a = X.relax(s.rows, wr, nu, s.g.n_fft, cycles=3)
    b = X.relax(s.rows, wr, nu, s.g.n_fft, cycles=3, schedule="cluster")
    assert a.nu.tobytes() == b.nu.tobytes() and a.residual.tobytes() == b.residual.tobytes() and a.decisions.tobytes() == b.decisions.tobytes()
    assert np.abs(a.nu - nu).max() > 0


def test_residual_energy_does_not_rise_on_one_row():
    """span_rows = 0, both tones on one row: every re-fit is a least-squares fit at a frequency that raises the restored tone's periodogram, so sum |R|^2 falls (or, to
    rounding, stays) from cycle to cycle."""
    s = X.oracle_rows("a4_L28")
    r = X.run("pair", s.rows, span_rows=0)
    e = r.energy
    print(f"energy after step 0 and each cycle, relative to the first: {(e / e[0]).tolist()}")
    assert r.decisions.all() and (np.diff(e) <= 1e-13 * e[0]).all() and e[-1] < e[0]
    t = X.relax(X.tone_rows(28, (0.011, 0.011 + 1.3 / 28), (1.0, 0.5)), [0, 0], [0.0115, 0.0575], 64, span_rows=0)
    assert (np.diff(t.energy) <= 1e-13 * t.energy[0]).all() and t.energy[-1] <= 1e-20 * t.energy[0]


def test_every_bracket_decision_is_well_conditioned():
    """Every case tests/test_gpu_relax.py runs, every cycle, every entry: |P'| at both ends of the box against the size of the terms that form it (the module's
    docstring) is 1e-6 or more -- about 1e7 times the rounding of the device's fp64 sums.  Cases with a failed bracket (status 1) are among them."""
    worst, failed = np.inf, 0
    for case in X.CASES:
        r = X.oracle_relax(case)
        row, _ = X.entries(case)
        m = float(r.margins.min()) if r.margins.size else np.inf
        print(f"{case}: {row.size} entries, {r.decisions.shape[0]} cycles: smallest margin {m:.3e}; {int((~r.decisions).sum())} brackets failed; status {r.status.tolist()}")
        assert m >= MARGIN, case
        worst, failed = min(worst, m), failed + int((~r.decisions).sum())
    print(f"smallest margin of all: {worst:.3e}")
    assert failed > 0 and X.oracle_relax("off_the_lobe").status.tolist() == [1] and X.oracle_relax("edge_rows").status.tolist() == [0, 1, 0]
    assert {len(X.entries(c)[0]) for c in X.CASES} >= {1, 2, 3, 5, 64}
    assert {(X.n_symbols(s), X.SCENES[s]["n_ants"]) for s in X.SCENES} >= {(28, 4), (29, 1), (28, 65), (280, 4), (56, 4)} and X.is_upa("upa2x2_L28")


def test_end_to_end_on_the_oracle_chain():
    """O.mono_static_sensing at 24 PRB, 16 elements, two targets at one range whose tones lie 1.8 lobes apart (+-0.9 lobes: +-38.6 m/s), amplitudes 1 : 0.5.  The
    restatement of cleanTargets extracts both; its velocities are off by 0.14 and 0.81 m/s, the re-fit of its two entries by 0.13 and 0.11 m/s: the largest error falls
    from 0.81 to 0.13 m/s (what is left is noise and the uneven cyclic prefix, which a tone model does not hold)."""
    s = X.oracle_rows("e2e_a16")
    c = K.clean(s.rows, s.g, max_iter=8)
    kept = np.flatnonzero(c.parent == np.arange(c.n_iter))
    assert kept.size == 2 and (c.row[kept] == X.TARGET_ROW).all() and (c.status == 0).all()
    sep = abs(s.nu[0] - s.nu[1]) * s.L
    assert 1.3 <= sep <= 2.0
    r = X.relax(s.rows, c.row[kept] - s.g.first_row, c.nu[kept], s.g.n_fft)
    truth = np.array([K.true_velocity(s.rp, q) for q in range(2)])
    f = s.g.n_fft * s.g.v_res
    e_seq = [float(np.abs(c.nu[kept] * f - t).min()) for t in truth]
    e_relax = [float(np.abs(r.nu * f - t).min()) for t in truth]
    print(f"tones {sep:.2f} lobes apart; velocity errors: sequential {np.round(e_seq, 4).tolist()}, re-fitted {np.round(e_relax, 4).tolist()} m/s; margins {r.margins.min():.3e}")
    assert (r.status == 0).all() and r.last_step.max() <= 1e-9 and r.margins.min() >= MARGIN
    assert max(e_relax) <= max(e_seq)
    assert max(e_relax) <= 0.5 * max(e_seq)                                # the visible gap: measured 0.13 against 0.81 m/s


def test_binding_has_the_prototype_and_the_abi_is_unchanged(binding):
    """include/isac_relax.h is additive under ABI 8: no new struct, no new isac_abi_sizeof selector; the header carries the defaults and the rule's key words, isac_clean.h
    points to it, and its one function refuses a NULL context.  (Its prototype line is compared with the header by tests/test_abi_cpu.py, row "isac_relax.h".)"""
    L = binding
    hdr = open(os.path.join(ROOT, "include", "isac_relax.h")).read()
    plain = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    assert "typedef" not in plain and "ISAC_SIZEOF" not in plain
    for macro, want in (("CYCLES", X.CYCLES), ("BOX", X.BOX), ("MAX_TONES", 64)):
        assert float(re.search(rf"#define ISAC_RELAX_{macro} ([0-9.]+)", plain).group(1)) == want
    assert L.ISAC_RELAX_MAX_TONES == 64
    for word in ("OUT OF SCOPE", "MEX", "SCHEDULE", "bit for bit", "sincos of the full argument", "(q0 + q1) + (q2 + q3)", "halved 40 times", "a refused call writes nothing"):
        assert word in hdr, word
    assert "isac_relax.h" in open(os.path.join(ROOT, "include", "isac_clean.h")).read()
    lib = L.load()                                                             # (needs no GPU)
    assert lib.isac_abi_version() == 8 == L.ISAC_ABI_VERSION and lib.isac_abi_sizeof(13) == -1
    assert lib.isac_fft2d_relax_targets(None, None, None, 0, 16, 2, 0.5, *([None] * 11)) == 1   # refused before anything touches a device: no context
    assert callable(load_pkg().sensing.estimation.relaxTargets)
