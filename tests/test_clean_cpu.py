"""isac_fft2d_clean_targets (project-defined, include/isac_clean.h) without a GPU: the conditioning of every case tests/test_gpu_clean.py runs and the outcomes of the loop,
on the oracle alone; the restatement's step 8; the binding's prototype line.  The device library is not asked for anything but its symbol table."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_pkg

import _clean_restatement as K

MARGIN = 1e-6


def _cells(r):
    return list(zip(r.row.tolist(), r.col.tolist()))


@pytest.mark.parametrize("case", list(K.CASES))
def test_case_conditioning(case):
    """Every margin of every decision of every pass -- CFAR, local maximum, refine step 2, parent distance -- is at least 1e-6, and every case that max_iter does not stop
    ends with an empty list."""
    s, r = K.oracle_rows(K.CASES[case][0]), K.oracle_clean(case)
    print(f"{case}: list of the CPI {s.cells} -> cells {_cells(r)} hits {r.hits.tolist()} parent {r.parent.tolist()} n_left {r.n_left}; bins "
          f"{(r.nu * s.g.n_fft + s.g.n_fft // 2 + 1).round(3).tolist()}")
    for j, m in enumerate(r.margins):
        print(f"  pass {j}: {len(r.lists[j])} cells; margins det {m.det:.3e} max {m.max:.3e} near {m.near:.3e} step 2 {m.m2:.3e} parent {m.parent:.3e}")
    assert K.min_margin(r) >= MARGIN
    assert r.n_iter >= 1 and (r.status == 0).all() and (r.hits >= 1).all()
    if "max_iter" in K.CASES[case][1]:                                      # stopped by max_iter: the closing pass still lists cells
        assert r.n_iter == K.CASES[case][1]["max_iter"] and r.n_left >= 1
    else:
        assert r.n_iter < K.MAX_ITER and r.n_left == 0
    assert len(r.margins) == r.n_iter + 1 and r.residual.shape == s.rows.shape


def test_masked_target_is_found():
    """Both targets at 100 m, the second one 20 dB down: its cell (88, 124) is not in the list of the CPI -- whose other two entries are sidelobes of the first -- and is the
    second entry of the result; its refined velocity is closer to the truth than the grid velocity of ANY listed entry."""
    s, r = K.oracle_rows("masked"), K.oracle_clean("masked")
    assert s.cells == [(88, 134), (88, 123), (88, 118)] and K.MASKED_CELL not in s.cells
    assert _cells(r) == [(88, 134), K.MASKED_CELL] and r.hits[1] >= 1 and r.n_kept == 2 and r.parent.tolist() == [0, 1]
    truth = K.true_velocity(s.rp, 1)
    listed = (s.list.col - s.g.n_fft / 2 - 1) * s.g.v_res
    print(f"truth {truth:.4f} m/s; refined {r.vel[1]:.4f}; listed (grid) {listed.round(4).tolist()}")
    assert abs(r.vel[1] - truth) < np.abs(listed - truth).min()
    bins = r.nu * s.g.n_fft + s.g.n_fft // 2 + 1
    assert np.abs(bins - [133.460, 124.502]).max() < 5e-4                  # the figures of the NumPy prototype the rule was settled on


def test_gap_scene_needs_the_mask():
    """With the 'S' slot silent the list of the CPI holds the gap lobes (7 and 6 bins from the peak).  The tone fitted on the 42 transmitted symbols: both targets, then
    empty.  Fitted on all 56: the strong target alone, then empty -- the weak one stays hidden under the residue."""
    s = K.oracle_rows("masked_gap")
    assert s.cells == [(88, 134), (88, 127), (88, 140)]
    with_mask, without = K.oracle_clean("masked_gap"), K.oracle_clean("masked_gap_nomask")
    assert _cells(with_mask) == [(88, 134), K.MASKED_CELL] and with_mask.n_left == 0 and with_mask.n_kept == 2
    assert _cells(without) == [(88, 134)] and without.n_left == 0
    silent = s.rows[:, 42:, :]
    assert not silent.any() and with_mask.residual[:, 42:, :].tobytes() == silent.tobytes()   # the silent symbols are not touched


def test_row_span():
    """Span 0 stops after one entry (the rows +-1 still mask the weak target); span 1 finds it, then lists the strong target's residues two rows away; span 2 gives the two
    targets and stops -- hence the default."""
    assert _cells(K.oracle_clean("masked_span0")) == [(88, 134)]
    assert _cells(K.oracle_clean("masked_span1")) == [(88, 134), K.MASKED_CELL, (90, 134), (86, 134)]
    assert _cells(K.oracle_clean("masked")) == [(88, 134), K.MASKED_CELL]
    s = K.oracle_rows("masked")
    three = K.clean(s.rows, s.g, span_rows=3)
    assert _cells(three) == [(88, 134), K.MASKED_CELL] and three.n_left == 0


def test_split_scene_gives_exactly_two():
    """split273: 6 listed entries for 2 targets -> exactly 2 kept entries and an empty list; the refined bins of the prototype."""
    s, r = K.oracle_rows("split273"), K.oracle_clean("split273")
    assert len(s.cells) == 6 and _cells(r) == [(88, 133), (152, 121)] and r.n_kept == 2 and r.n_left == 0
    bins = r.nu * s.g.n_fft + s.g.n_fft // 2 + 1
    assert np.abs(bins - [135.676, 117.863]).max() < 5e-4


@pytest.mark.parametrize("scene", ["a4_273prb", "a8_273prb", "a4_24prb_generic", "a4_24prb_truncated", "split24"])
def test_clear_scenes_keep_their_two_cells(scene):
    """Where the list already holds the two targets first, the loop returns those two cells and stops."""
    s, r = K.oracle_rows(scene), K.oracle_clean(scene)
    assert _cells(r) == s.cells[:2] and r.n_left == 0 and r.n_kept == 2
    assert {round(float(t["Range"]) / s.g.r_res) for t in s.rp.targetRealPos} == {int(x) - 1 for x in r.row}


def test_max_iter_and_merge_tol():
    """max_iter = 1 leaves n_left = the size of the second pass's list; merge_tol = 0 keeps every entry, a wide one makes the second entry a residue -- which is still
    subtracted, so the residual rows are the same bytes."""
    s = K.oracle_rows("split273")
    full, one = K.oracle_clean("split273"), K.clean(s.rows, s.g, max_iter=1)
    assert one.n_iter == 1 and one.n_left == len(full.lists[1]) == 3 and _cells(one) == _cells(full)[:1]
    assert K.oracle_clean("split273_one").n_left == 3 and K.oracle_clean("masked_tol0").parent.tolist() == [0, 1]   # the two cases the device runs
    s = K.oracle_rows("masked")
    base, wide, off = K.oracle_clean("masked"), K.oracle_clean("masked_bigtol"), K.clean(s.rows, s.g, merge_tol=0.0)
    assert wide.parent.tolist() == [0, 0] and wide.n_kept == 1 and wide.n_iter == 2
    assert off.parent.tolist() == [0, 1] and off.n_kept == 2
    for r in (wide, off):
        assert r.nu.tobytes() == base.nu.tobytes() and r.residual.tobytes() == base.residual.tobytes()


def test_cancel_removes_a_tone_on_the_active_symbols():
    """Step 8 of the restatement on a synthetic row: an exact tone on the active symbols is removed to rounding, the inactive symbols keep their bytes, and what is
    orthogonal to the tone stays."""
    rng = np.random.default_rng(5)
    L, A, nu = 56, 3, 0.1234
    l = np.arange(L)
    amp = rng.standard_normal(A) + 1j * rng.standard_normal(A)
    tone = np.exp(2j * np.pi * nu * l)[:, None] * amp[None, :]
    y = tone.copy()
    y[42:] = 7.0
    out = K.cancel_ld(y, nu, K.GAP_MASK).astype(np.complex128)
    assert np.abs(out[:42]).max() <= 1e-14 and out[42:].tobytes() == y[42:].tobytes()
    again = K.cancel_ld(out, nu, K.GAP_MASK).astype(np.complex128)
    assert np.abs(again - out).max() <= 1e-14                             # the fit of a residual is zero: a projection
    assert list(K.span_of(88, 1, 376, 2)) == [85, 86, 87, 88, 89] and list(K.span_of(1, 1, 376, 2)) == [0, 1, 2] and list(K.span_of(376, 1, 376, 2)) == [373, 374, 375]


def test_binding_has_the_prototype_and_the_abi_is_unchanged():
    """include/isac_clean.h is additive under ABI 8: no new struct, no new isac_abi_sizeof selector; the header carries the defaults, the rule's key words and what is out
    of scope, and its one function refuses a NULL context.  (Its prototype line is compared with the header by tests/test_abi_cpu.py, row "isac_clean.h".)"""
    import __graft_entry__ as g
    g.build()
    L = load_pkg()._lib
    hdr = open(os.path.join(ROOT, "include", "isac_clean.h")).read()
    plain = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    assert "typedef" not in plain and "ISAC_SIZEOF" not in plain
    for macro, want in (("SPAN_ROWS", 2), ("MERGE_TOL", 0.5)):
        assert float(re.search(rf"#define ISAC_CLEAN_{macro} ([0-9.]+)", plain).group(1)) == want
    for word in ("OUT OF SCOPE", "MEX", "deriving sym_active", "RELAX", "beam planes", "range-sidelobe model", "sincos of the full argument", "(q0 + q1) + (q2 + q3)"):
        assert word in hdr, word
    lib = L.load()                                                             # (needs no GPU)
    assert lib.isac_abi_version() == 8 == L.ISAC_ABI_VERSION and lib.isac_abi_sizeof(13) == -1
    fn = lib.isac_fft2d_clean_targets
    assert fn(None, None, 8, 2, 0.5, *([None] * 18)) == 1                   # refused before anything touches a device: no context
    est = load_pkg().sensing.estimation
    assert callable(est.cleanTargets)
