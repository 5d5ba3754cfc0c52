"""tests/_cfar_band_cases.py on the oracle alone (no GPU): every scene's window lies inside the map, the restated host rules put every case on the side of each limit the
table claims, the table as a whole reaches both sides of all five panel-detector limits, all three Doppler kernels, a refused and a quiet zone, and every case clears the 1e-9
decision margin at its own bands -- the condition under which tests/test_gpu_cfar_bands.py compares lists exactly with nothing skipped."""
from __future__ import annotations

import numpy as np
import pytest

import _cfar_band_cases as T

ALL_CASES = list(T.CASES) + [T.RANGE_WINDOW_CASE]


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_case_sits_where_the_table_says(case):
    o = T.oracle_of(case)
    sc, g = o.sc, o.geom
    assert (int(sc.rp.nFFT), int(sc.rp.nIFFT)) == (case.n_fft, case.n_ifft)
    assert (g.gr, g.gc) == case.guard and (g.hr - g.gr, g.hc - g.gc) == case.train
    assert T.inside_map(g, case.n_ifft, case.n_fft), "window leaves the map"
    assert g.first_row >= 1 and g.first_col >= 1 and g.first_row + g.nr - 1 <= case.n_ifft and g.first_col + g.nc - 1 <= case.n_fft
    lim, pp = T.panel_limits(g)
    for name, side in case.limits.items():
        assert lim[name] is side, f"{name}: {lim}"
        if side is False and name != "pr":                       # just outside that limit and no other
            assert [k for k, v in lim.items() if v is False] == [name]
    have = dict(n_cut_rows=g.n_cut_rows, n_cut_cols=g.n_cut_cols, nc=g.nc, pr=pp.pr, n_panels=pp.n_panels)
    for name, n in case.counts.items():
        assert have[name] == n, f"{name}: {have}"
    assert T.detector_of(g, True) == case.detector and T.detector_of(g, False) == case.unfused
    assert T.doppler_kernel_of(g, case.n_fft) == case.doppler
    n_det = [d.shape[1] for d in o.dbg.detections]
    if case.kind == "quiet":
        assert n_det == [0] * sc.A and o.est is None
    else:
        assert min(n_det) >= 1 and o.est is not None, n_det
    for a in range(sc.A):
        assert T.guard_band_ok(np.abs(o.dbg.rdm[:, :, a]) ** 2, o.cfg.CUTIdx, o.cfg.Pfa, case.guard, case.train, 1e-9), f"antenna {a}: margin {o.margin[a]:.3e}"
    print(f"{case.name}: margin {min(o.margin):.3e}, detections {n_det}")


def test_table_reaches_every_side():
    cases = T.CASES
    # the five panel-detector limits, from both sides; the side is the restated rule's, not the table's word
    for name in T.LIMITS:
        sides = {T.panel_limits(T.oracle_of(c).geom)[0][name] for c in cases if name in c.limits}
        assert sides == {True, False}, name
    tally = {name: [sum(1 for c in cases if T.panel_limits(T.oracle_of(c).geom)[0][name] is s) for s in (True, False)] for name in T.LIMITS}
    print("cases inside / outside each limit:", tally)
    # exactly at the limit on the inside, one step beyond on the outside
    at = {c.name: (T.oracle_of(c).geom, T.panel_limits(T.oracle_of(c).geom)[1]) for c in cases if c.limits}
    g, p = at["pr8_panel"]; assert p.pr == 8
    g, p = at["pr6_window"]; assert p.pr == 6
    g, p = at["prcols_2040"]; assert p.pr * g.n_cut_cols <= 2048 < p.pr * (g.n_cut_cols + 1)
    g, p = at["prcols_2064"]; assert p.pr * (g.n_cut_cols - 1) <= 2048 < p.pr * g.n_cut_cols
    assert at["nc_128"][0].nc == 128 and at["nc_130"][0].nc == 130 and at["nc_128"][0].n_cut_cols == at["nc_130"][0].n_cut_cols
    assert at["panels_256"][1].n_panels == 256 and at["panels_257"][1].n_panels == 257
    g, p = at["segments_4096"]; assert g.n_cut_cols * p.n_panels == 4096
    g, p = at["segments_4352"]; assert (g.n_cut_cols - 1) * p.n_panels == 4096
    # kernels and outcomes
    assert {c.doppler for c in cases} == {"pow", "fft256_pruned", "fft256_full"}
    assert {c.n_ifft for c in cases} == {512, 4096}
    assert {(c.n_ifft, c.n_fft) for c in cases if c.name.startswith("nrb")} == {(512, 64), (512, 256), (4096, 256)}
    assert {c.detector for c in cases} == {"panel", "window", "refused"} and {c.kind for c in cases} == {"detect", "quiet", "refused"}
    # asymmetry in both orders, a zero guard and a zero training size in one dimension only
    geoms = [T.oracle_of(c).geom for c in cases if c.kind == "detect"]
    assert any(g.hr < g.hc and g.gr < g.gc for g in geoms) and any(g.hr > g.hc and g.gr > g.gc for g in geoms)
    assert any(g.gr == 0 and g.gc > 0 for g in geoms) and any(g.hr == g.gr and g.gr > 0 and g.hc > g.gc for g in geoms)
    # the window detector's column loop: more CUT columns than one pass holds
    g = T.oracle_of(T.CASE["dense_long_zone"]).geom
    assert 1 <= T.window_panel(g) < g.n_cut_cols
    # dense lists: every (column, panel) segment of the merge holds a detection
    o = T.oracle_of(T.CASE["dense_default_zone"])
    g, p = o.geom, T.panel_limits(o.geom)[1]
    for det in o.dbg.detections:
        seg = set(zip((det[1] - g.col0).tolist(), ((det[0] - g.row0) // p.pr).tolist()))
        assert len(seg) == g.n_cut_cols * p.n_panels and det.shape[1] > 4096
    o = T.oracle_of(T.CASE["dense_long_zone"])                   # (the strong target's own cells keep a few of its 468 segments empty)
    assert o.dbg.detections[0].shape[1] > 4096
    # the refused zone: neither detector, and the same zone at the default bands is taken by both
    o = T.oracle_of(T.CASE["refused"])
    assert T.window_panel(o.geom) < 1 and T.panel_limits(o.geom)[0]["pr"] is False
    gd = T.window_geometry(o.cfg.CUTIdx, *T.DEFAULT_BANDS)
    assert T.detector_of(gd, True) == "panel" and T.detector_of(gd, False) == "window"
    smallest = min((min(T.oracle_of(c).margin), c.name) for c in cases)
    print(f"smallest guard margin over the table: {smallest[0]:.3e} ({smallest[1]})")
    assert smallest[0] >= T.MARGIN_FLOOR > T.MARGIN


@pytest.mark.parametrize("name", T.DEFAULT_BAND_RERUNS)
def test_default_band_reruns_are_decidable(name):
    """The GPU tests run these scenes once more at the default bands on contexts that have just seen other bands: detections on every antenna, both detectors available, 1e-9."""
    o = T.oracle_of(T.CASE[name], default_bands=True)
    assert (o.cfg.GuardBandSize, o.cfg.TrainingBandSize) == T.DEFAULT_BANDS and (o.geom.hr, o.geom.hc) == (3, 3)
    assert T.detector_of(o.geom, True) == "panel" and T.detector_of(o.geom, False) == "window" and o.est is not None
    assert min(d.shape[1] for d in o.dbg.detections) >= 1
    for a in range(o.sc.A):
        assert T.guard_band_ok(np.abs(o.dbg.rdm[:, :, a]) ** 2, o.cfg.CUTIdx, o.cfg.Pfa, *T.DEFAULT_BANDS, 1e-9), f"antenna {a}: margin {o.margin[a]:.3e}"


def test_range_window_case_spans_two_blocks_where_its_cut_rows_span_one():
    o = T.oracle_of(T.RANGE_WINDOW_CASE)
    g = o.geom
    win, cut = T.row_blocks(g)
    assert cut == (1, 1) and win == (0, 1) and g.hr != g.hc and g.hr == 12
    rows = o.cfg.CUTIdx[0]
    assert rows.min() - 1 >= 512 > rows.min() - g.hr - 1 and rows.max() + g.hr - 1 < 1024


def test_range_window_case_is_decidable_under_the_seeded_spectral_noise():
    """The cached and the fused range routes draw their own (Philox) noise: the same scene with that field restated clears the margin with decades to spare over the 1e-7 of
    the noise level by which the device's float32 Box-Muller may differ from the restatement."""
    o = T.spectral_reference_of(T.RANGE_WINDOW_CASE)
    print(f"margins under the restated spectral field: {['%.2e' % m for m in o.margin]}")
    assert min(o.margin) > 1e-6 and o.est is not None and min(d.shape[1] for d in o.dbg.detections) > 1000


def test_window_detector_iteration_clamp_is_unreachable():
    """isac_cfar_window halves nothing: its `n_cut_rows * panel > 32 * 1024` clamp cannot fire, because the LDS budget already bounds the staged window -- panel + 2 hc columns of
    nr >= n_cut_rows doubles in 128 KiB -- to 16384 cells."""
    for nr in range(1, 4097):
        for hc in (0, 1, 3):
            panel = T.LDS_BUDGET // (8 * nr) - 2 * hc
            assert panel < 1 or nr * panel <= 16384
