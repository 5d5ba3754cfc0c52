"""isac_fft2d_beam_clean_targets (project-defined, include/isac_beam_clean.h) without a GPU: the conditioning of every case tests/test_gpu_beam_clean.py runs and the
outcomes of the loop, on the oracle alone; the capability the call adds over cleanTargets and beamDetect; the binding's prototype line and its host-side argument checks.
The device library is not asked for anything but its symbol table."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_pkg

import _beam_clean_restatement as BC
import _beam_detect_restatement as B
import _clean_restatement as K

MARGIN = 1e-6          # the project's floor


def _cells(r):
    return list(zip(r.row.tolist(), r.col.tolist()))


@pytest.mark.parametrize("case", list(BC.CASES))
def test_case_conditioning(case):
    """Every margin of every decision of every pass -- CFAR on every beam plane, local maximum, the order of the list, b* of the picked cell, refine step 2, parent distance
    -- is at least 1e-6, and every case that max_iter does not stop ends with an empty list."""
    scene, beams, _ = BC.CASES[case]
    s, r = BC.oracle_rows(scene), BC.oracle_beam_clean(case)
    kw = BC.keywords(case, s.g)
    print(f"{case}: cells {_cells(r)} beam {r.beam.tolist()} hits {r.hits.tolist()} parent {r.parent.tolist()} n_left {r.n_left}; vel {r.vel.round(3).tolist()}")
    for j, m in enumerate(r.margins):
        print(f"  pass {j}: {len(r.lists[j])} cells; margins " + " ".join(f"{k} {getattr(m, k):.3e}" for k in BC.MARGIN_KEYS))
    assert BC.min_margin(r) >= MARGIN
    assert r.n_iter >= 1 and (r.status == 0).all() and (r.hits >= 1).all() and r.beam.min() >= 1 and r.beam.max() <= BC.weights(scene, beams)[0].shape[1]
    if "max_iter" in kw:                                                    # stopped by max_iter: the closing pass still lists cells
        assert r.n_iter == kw["max_iter"] and r.n_left >= 1 and r.left_cells.shape == (r.n_left, 2)
    else:
        assert r.n_iter < BC.MAX_ITER and r.n_left == 0 and r.left_cells.shape == (0, 2)
    assert len(r.margins) == r.n_iter + 1 and r.residual.shape == s.rows.shape and r.beam_pow.shape[:1] == (s.g.n_rows,)
    assert len(BC.touched_rows(r, s.g, kw.get("span_rows", 2))) >= 1


def test_the_cases_cover_what_the_band_update_can_get_wrong():
    """Spans 0, 1, 2 and the whole window (clipped at both edges); one beam, 5, 16, 37 and the whole scan grid of 361; 4, 6, 8, 16 elements and a planar array; every
    detector; the mask; max_iter = 1; merge_tol 0 and wide."""
    kws = {c: BC.keywords(c, BC.oracle_rows(BC.CASES[c][0]).g) for c in BC.CASES}
    assert {kw.get("span_rows", 2) for kw in kws.values()} >= {0, 1, 2, BC.oracle_rows("a4_24prb_generic").g.n_rows}
    assert {b for _, b, _ in BC.CASES.values()} == {"b1", "b5", "b16", "b37", "b361"}
    assert {BC.make(s).A for s in BC.SCENES} == {4, 6, 8, 16} and any(BC.is_upa(s) for s in BC.SCENES)
    assert {kw.get("method", "CA") for kw in kws.values()} == {"CA", "GOCA", "SOCA", "OS"}
    assert any("sym_active" in kw for kw in kws.values()) and {kw.get("merge_tol", 0.5) for kw in kws.values()} == {0.0, 0.5, 1e6}
    assert BC.oracle_beam_clean("cap8_one").n_left == 1 and BC.oracle_beam_clean("cap8_bigtol").parent.tolist() == [0, 0]
    wide, base = BC.oracle_beam_clean("cap8_bigtol"), BC.oracle_beam_clean("cap8")
    assert wide.n_kept == 1 and wide.residual.tobytes() == base.residual.tobytes()   # a residue is still subtracted
    allrows = BC.oracle_beam_clean("a4_24prb_generic_allrows")
    s = BC.oracle_rows("a4_24prb_generic")
    assert BC.touched_rows(allrows, s.g, s.g.n_rows) == list(range(s.g.n_rows))


def _capability(scene):
    """(cleanTargets' restatement, beamDetect's restatement, the loop) on a capability scene with the beam set b5 and CA at the stored pfa."""
    s = BC.oracle_rows(scene)
    W, azi = BC.weights(scene, "b5")
    clean = K.clean(s.rows, s.g, max_iter=8)
    P = BC.planes_of_rows(s.rows, s.g, W)
    return s, clean, BC.cells_of_planes(P, s.g), BC.beam_clean(s.rows, s.g, W, beam_azi=azi, max_iter=8)


def test_capability_scene_gives_the_table():
    """8 elements, both targets at 100 m, the second echo 30 dB down (it needs the 9 dB of the array): the element-wise loop lists (88, 134) only; the beam planes of the one
    map list (88, 134) and the sidelobe cell (88, 122), not the weak target's cell (88, 124); the loop on beam planes gives (88, 134) on beam 4, then (88, 124) on beam 2
    with a velocity within half a metre per second of the truth, and an empty list."""
    s, clean, bd, r = _capability(BC.CAP)
    weak = BC.CAP_CELLS[1]
    assert _cells(clean) == [(88, 134)] and clean.n_left == 0
    assert _cells(bd) == [(88, 134), (88, 122)] and weak not in _cells(bd)
    assert _cells(r) == BC.CAP_CELLS and r.beam.tolist() == [4, 2] and r.n_left == 0 and r.n_kept == 2 and r.n_iter == 2
    truth = BC.true_velocity(s.rp, 1)
    grid = (bd.col - s.g.n_fft / 2 - 1) * s.g.v_res
    print(f"truth {truth:.4f} m/s; loop {r.vel[1]:.4f}; beam planes of the one map (grid) {grid.round(4).tolist()}; smallest margin {BC.min_margin(r):.3e}")
    assert abs(truth - -20.86) < 5e-3 and abs(r.vel[1] - -20.49) < 5e-3 and abs(r.vel[1] - truth) < np.abs(grid - truth).min()
    assert abs(BC.min_margin(r) - 7.7e-3) < 1e-4
    assert BC.oracle_beam_clean("cap8").nu.tobytes() == r.nu.tobytes()      # the case the device runs is this loop


@pytest.mark.parametrize("scene,second,margin", [("cap8_s22", (88, 124), 1.8e-2), ("cap8_s23", (88, 125), 4.4e-3)])
def test_capability_holds_for_other_seeds(scene, second, margin):
    """Other data and noise: the same two entries (the weak target's cell moves by at most one bin), an empty list, and the margins of the prototype the rule was settled on."""
    s, clean, bd, r = _capability(scene)
    assert _cells(r) == [(88, 134), second] and r.n_left == 0 and second not in _cells(clean) and second not in _cells(bd)
    print(f"{scene}: smallest margin {BC.min_margin(r):.3e}")
    assert BC.min_margin(r) >= MARGIN and abs(BC.min_margin(r) / margin - 1) < 0.06


def test_gap_scene_needs_the_mask():
    """With the 'S' slot silent, the tone fitted on the 42 transmitted symbols uncovers the second target; fitted on all 56 it does not."""
    with_mask, without = BC.oracle_beam_clean("masked_gap"), BC.oracle_beam_clean("masked_gap_nomask")
    assert _cells(with_mask) == [(88, 134), K.MASKED_CELL] and with_mask.n_left == 0 and _cells(without) == [(88, 134)] and without.n_left == 0
    silent = BC.oracle_rows("masked_gap").rows[:, 42:, :]
    assert not silent.any() and with_mask.residual[:, 42:, :].tobytes() == silent.tobytes()   # the silent symbols are not touched


def test_binding_has_the_prototype_and_the_abi_is_unchanged():
    """include/isac_beam_clean.h is additive under ABI 8: no new struct, no new macro, no new isac_abi_sizeof selector; the header carries the rule's key words and what is
    out of scope, isac_clean.h still names the gap this call closes, and its one function refuses a NULL context.  (Its prototype line is compared with the header by
    tests/test_abi_cpu.py, row "isac_beam_clean.h".)"""
    import __graft_entry__ as g
    g.build()
    L = load_pkg()._lib
    hdr = open(os.path.join(ROOT, "include", "isac_beam_clean.h")).read()
    plain = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    assert "typedef" not in plain and "ISAC_SIZEOF" not in plain and "#define ISAC_" not in plain.replace("#define ISAC_BEAM_CLEAN_H", "")
    for word in ("OUT OF SCOPE", "MEX", "beamformed series", "spatial sidelobes", "THE BAND UPDATE", "bit for bit", "sincos of the full argument", "(q0 + q1) + (q2 + q3)",
                 "ascending a from 0", "never contracted", "On an error no output is written", "The arguments are checked first, the CPI second"):
        assert word in hdr, word
    lib = L.load()                                                             # (needs no GPU)
    assert lib.isac_abi_version() == 8 == L.ISAC_ABI_VERSION and lib.isac_abi_sizeof(13) == -1
    fn = lib.isac_fft2d_beam_clean_targets
    assert fn(None, None, 5, None, None, 8, 2, 0.5, *([None] * 22)) == 1     # refused before anything touches a device: no context
    assert "cancellation on beam planes" in open(os.path.join(ROOT, "include", "isac_clean.h")).read()


class _NoCpi:
    """A context whose library answers the size query like a completed 4-element CPI and must not be asked for anything else."""
    fft2d_grid_shape = (288, 28, 4)
    handle = None

    class lib:                                                               # noqa: N801
        @staticmethod
        def isac_fft2d_get_power_window(h, p, cap, dims, fr, fc):
            dims[0], dims[1], dims[2] = 55, 15, 4
            return 0

        @staticmethod
        def isac_fft2d_beam_clean_targets(*a):
            raise AssertionError("the host-side checks come first")

    @staticmethod
    def check(st):
        assert st == 0


def test_host_side_argument_checks():
    """sensing.estimation.beamClean refuses, before the library is called: weights that are not [A x B], labels that are not one per beam, a mask or a symbol count that
    contradicts the CPI, an unknown detector."""
    est = load_pkg().sensing.estimation
    assert callable(est.beamClean)
    W = np.ones((4, 5), dtype=np.complex128)
    for bad in (dict(W=W[:3]), dict(W=W[:, 0]), dict(W=W, beam_azi=np.zeros(4)), dict(W=W, symActive=np.ones(29)), dict(W=W, residual=True, nSymbols=29),
                dict(W=W, symActive=np.ones(29), nSymbols=29), dict(W=W, Method="XX"), dict(W=W, ThresholdFactor="Custom"), dict(W=W, ThresholdFactor="Input port")):
        with pytest.raises(ValueError):
            est.beamClean(_NoCpi, bad.pop("W"), **bad)
    ctx = type("NoShape", (_NoCpi,), {"fft2d_grid_shape": None})
    with pytest.raises(ValueError):                                           # no recorded grid shape: symActive and residual need nSymbols
        est.beamClean(ctx, W, symActive=np.ones(28))
    with pytest.raises(ValueError):
        est.beamClean(ctx, W, residual=True)
