"""isac_fft2d_refine_targets on the MI355X: off-grid Doppler, split-lobe merge and sidelobe flags for a target list of the last fft2D (project-defined --
include/isac_refine.h).

Scenes and the oracle-only result come from tests/_refine_restatement.py; tests/test_refine_cpu.py has shown on the oracle that every decision in them clears its margin
by 1e-6 or more (the measured minimum is 1.1e-3), so nothing here is left out or skipped.  Each scene runs once per module."""
from __future__ import annotations

import ctypes as C
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import make_scene

import _beam_detect_restatement as B
import _refine_restatement as R
import _target_list_restatement as T
import _target_list_upa_restatement as TU

pytestmark = pytest.mark.gpu

NU_TOL = 1e-6          # |nu_dev - nu_ref| L
FIELD_TOL = 1e-10      # the project's field tolerance
OUT_KEYS = ("rng", "vel", "azi", "power", "row", "col", "nu", "status", "n_merged", "sidelobe_of")


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context()
    c.set_upa_doa(True)
    yield c
    c.close()


def _blocks(pkg, sc):
    rp = pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)
    return rp, pkg.sensing.detection.cfar2D(rp)


def _raw(c, row, col, merge_tol=0.5, merge_rows=1, margin=2.0, A=None, ele=True, n=None):
    """The C call itself: (status code, namespace of the raw outputs, input indices)."""
    row, col = np.ascontiguousarray(row, dtype=np.int32), np.ascontiguousarray(col, dtype=np.int32)
    n = row.size if n is None else n
    m = max(row.size, 1)
    o = SimpleNamespace(status=np.full(m, -7, dtype=np.int32), parent=np.full(m, -7, dtype=np.int32), sidelobe_of=np.full(m, -7, dtype=np.int32), nu=np.zeros(m),
                        vel=np.zeros(m), power=np.zeros(m), azi=np.zeros(m), ele=np.full(m, np.nan), snapshots=None if A is None else np.zeros((A, m), dtype=np.complex128, order="F"))
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)    # noqa: E731
    kept = C.c_int32(-1)
    st = c.lib.isac_fft2d_refine_targets(c.handle, p(row), p(col), n, merge_tol, merge_rows, margin, C.byref(kept), p(o.status), p(o.parent), p(o.sidelobe_of), p(o.nu),
                                         p(o.vel), p(o.power), p(o.azi), p(o.ele) if ele else None, p(o.snapshots))
    o.n_kept = int(kept.value)
    return st, o


_runs = {}


def _plain(pkg, ctx, name):
    """Scene `name` through monoStaticSensing -> isac_fft2d_dev -> the list -> the C call and sensing.estimation.refineTargets, once per module (host copies only)."""
    if name not in _runs:
        sc = R.make(name)
        rp, cf = _blocks(pkg, sc)
        cf = T.with_bands(name, cf)                                          # the default bands for every scene but T.BAND_SCENE
        est_mod = pkg.sensing.estimation
        d_txg, d_wave = ctx.to_device(sc.tx_grid), ctx.to_device(sc.tx_wave)
        echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=ctx)
        est, dbg = est_mod.fft2D(rp, cf, echo, d_txg, return_debug=True, ctx=ctx)
        tl = (est_mod.targetListUPA if R.is_upa(name) else est_mod.targetList)(ctx, snapshots=True)
        st, raw = _raw(ctx, tl["row"], tl["col"], A=sc.A)
        assert st == 0
        ref = est_mod.refineTargets(ctx, tl, snapshots=True)
        dbg_after = import_module(pkg.__name__ + ".sensing.estimation.fft2D").fft2D_debug(ctx, sc.A)
        tl_after = (est_mod.targetListUPA if R.is_upa(name) else est_mod.targetList)(ctx, snapshots=True)
        for d in (echo, d_txg, d_wave):
            d.free()
        _runs[name] = SimpleNamespace(sc=sc, rp=rp, cf=cf, est=est, dbg=dbg, dbg_after=dbg_after, tl=tl, tl_after=tl_after, raw=raw, ref=ref)
    return _runs[name]


def _same_out(a, b):
    assert a["n_in"] == b["n_in"]
    for k in OUT_KEYS + tuple(k for k in ("ele", "snapshots") if k in a or k in b):
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("name", list(R.SCENES))
def test_decisions_equal_the_restatement(pkg, ctx, name):
    """The list's cells are the oracle's; status, parent and sidelobe_of of the device equal the restatement's on the oracle's range rows, exactly; the Python dict is the
    kept entries in input order with sidelobe_of remapped."""
    r, s = _plain(pkg, ctx, name), R.oracle_scene(name)
    raw, want = r.raw, s.ref
    n = s.row.size
    print(f"{name}: rows {r.tl['row'].tolist()} cols {r.tl['col'].tolist()} -> status {raw.status.tolist()} parent {raw.parent.tolist()} sidelobe_of {raw.sidelobe_of.tolist()}")
    assert np.array_equal(r.tl["row"], s.row) and np.array_equal(r.tl["col"], s.col) and n >= R.MIN_ENTRIES.get(name, 2)
    assert np.array_equal(raw.status, want.status) and np.array_equal(raw.parent, want.parent) and np.array_equal(raw.sidelobe_of, want.sidelobe_of)
    assert raw.n_kept == want.n_kept
    kept = np.flatnonzero(want.parent == np.arange(n))
    d = r.ref
    assert d["n_in"] == n and np.array_equal(d["row"], s.row[kept]) and np.array_equal(d["col"], s.col[kept]) and np.array_equal(d["rng"], r.tl["rng"][kept])
    assert np.array_equal(d["n_merged"], np.bincount(want.parent, minlength=n)[kept]) and np.array_equal(d["status"], want.status[kept])
    pos = {int(i): j for j, i in enumerate(kept)}
    assert d["sidelobe_of"].tolist() == [pos.get(int(k), -1) for k in want.sidelobe_of[kept]]
    for k in ("nu", "vel", "power", "azi"):
        assert d[k].tobytes() == getattr(raw, k)[kept].tobytes(), k
    assert d["snapshots"].tobytes(order="F") == np.asfortranarray(raw.snapshots[:, kept]).tobytes(order="F")
    assert ("ele" in d) == R.is_upa(name) and (not R.is_upa(name) or d["ele"].tobytes() == raw.ele[kept].tobytes())


@pytest.mark.parametrize("name", list(R.SCENES))
def test_values_against_the_restatement(pkg, ctx, name):
    """|nu_dev - nu_ref| L <= 1e-6 against the long-double bisection; power within 1e-10 relative of P(nu_ref); vel = nu nFFT vRes."""
    r, s = _plain(pkg, ctx, name), R.oracle_scene(name)
    raw, want = r.raw, s.ref
    e_nu = np.abs(raw.nu - want.nu).max() * s.L
    e_p = np.abs(raw.power / want.power - 1).max()
    print(f"{name}: nu error {e_nu:.3e} / L, power error {e_p:.3e} relative; refined bins {(raw.nu * s.n_fft).round(4).tolist()}")
    assert e_nu <= NU_TOL
    assert e_p <= FIELD_TOL
    assert np.array_equal(raw.vel, raw.nu * s.n_fft * float(r.rp.vRes))


@pytest.mark.parametrize("name", list(R.SCENES))
def test_snapshots_and_direction(pkg, ctx, name):
    """x against the restatement's direct sum over the oracle's range rows at the DEVICE's own nu, to 1e-10 of max |x|; azi (and ele) = the lists' restatement of the
    Bartlett scan on the device's snapshots, exactly."""
    r, s = _plain(pkg, ctx, name), R.oracle_scene(name)
    raw = r.raw
    Y = s.rows_of(s.row)
    want = np.stack([R.spectrum(Y[i], raw.nu[i]) for i in range(s.row.size)], axis=1) / np.sqrt(float(s.n_fft))
    err = np.abs(raw.snapshots - want).max() / np.abs(want).max()
    print(f"{name}: snapshot error {err:.3e} of max |x|")
    assert err <= FIELD_TOL
    if R.is_upa(name):
        _, azi, ele, _, _ = TU.bartlett2d(raw.snapshots, r.sc.nV, r.sc.nH, r.rp)
        assert np.array_equal(raw.azi, azi) and np.array_equal(raw.ele, ele)
    else:
        _, azi, _, _ = T.bartlett(raw.snapshots, r.rp)
        assert np.array_equal(raw.azi, azi) and np.isnan(raw.ele).all()    # a ULA: ele is not written


def test_whole_chain_on_the_split_scene(pkg, ctx):
    """split273: 6 listed entries -> 5, 2 of them unflagged; getRMSE on those two gives a smaller velRMSE for both targets than any entry of the unrefined list does."""
    r = _plain(pkg, ctx, "split273")
    d = r.ref
    assert r.tl["row"].size == 6 and d["row"].size == 5
    clean = np.flatnonzero(d["sidelobe_of"] < 0)
    assert clean.size == 2
    getRMSE = pkg.sensing.postProcessing.getRMSE
    fine = getRMSE({k: d[k][clean] for k in ("rng", "vel", "azi")}, r.rp)
    coarse = getRMSE(r.tl, r.rp)
    truth_rng = np.array([float(t["Range"]) for t in r.rp.targetRealPos])
    seen = set()
    for j, i in enumerate(clean):
        q = int(np.flatnonzero(np.abs(truth_rng - d["rng"][i]) < r.rp.rRes)[0])
        same = np.flatnonzero(np.abs(r.tl["rng"] - truth_rng[q]) < r.rp.rRes)
        print(f"target {q + 1}: velRMSE refined {fine.velRMSE[j]:.4f} m/s, unrefined {coarse.velRMSE[same].round(4).tolist()}")
        assert fine.velRMSE[j] < coarse.velRMSE[same].min()
        seen.add(q)
    assert seen == {0, 1}


def test_routes_give_the_same_result(pkg, ctx):
    """Plain isac_fft2d_dev == fused + cached with a caller's echo grid == ISAC_OPT_TAIL_FUSION 0 / 1, byte for byte."""
    r = _plain(pkg, ctx, "split273")
    sc = r.sc
    est_mod = pkg.sensing.estimation
    c2 = pkg.Context()
    try:
        d_txg, d_wave = c2.to_device(sc.tx_grid), c2.to_device(sc.tx_wave)
        echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, r.rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, fuse_fft2d=(r.rp, r.cf, d_txg), ctx=c2)
        est_mod.fft2D(r.rp, r.cf, echo, d_txg, reuse_range=True, ctx=c2)
        _same_out(est_mod.refineTargets(c2, est_mod.targetList(c2), snapshots=True), r.ref)
        for tail in (False, True):
            c2.set_tail_fusion(tail)
            est_mod.fft2D(r.rp, r.cf, echo, d_txg, ctx=c2)
            _same_out(est_mod.refineTargets(c2, est_mod.targetList(c2), snapshots=True), r.ref)
    finally:
        c2.close()


def test_lazy_grid_gives_the_same_result(pkg):
    """A = 64, Q = 1, Philox spectral noise, L = 28 (~100 MB): the echo grid the context re-forms (never stored) against the stored one.  nFFT = 64 so that the
    28-symbol scene has detections at all."""
    sc = make_scene(n_ants=64, n_slots=2, num_slots_param=6, with_noise=False, zero_s_slots=False, seed=31)
    rp, cf = _blocks(pkg, sc)
    est_mod = pkg.sensing.estimation
    c = pkg.Context()
    try:
        d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
        kw = dict(nfft=4096, fuse_fft2d=(rp, cf, d_txg), ctx=c, seed=77, noise_domain="spectral")
        arr = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, **kw)
        est_mod.fft2D(rp, cf, arr, d_txg, reuse_range=True, ctx=c)
        stored = est_mod.refineTargets(c, est_mod.targetList(c), snapshots=True)
        lz = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, lazy=True, **kw)
        est_mod.fft2D(rp, cf, lz, d_txg, reuse_range=True, ctx=c)
        lazy = est_mod.refineTargets(c, est_mod.targetList(c), snapshots=True)
        assert stored["n_in"] >= 1 and (stored["status"] == 0).all()
        _same_out(lazy, stored)
    finally:
        c.close()


def test_input_from_other_lists_and_by_hand(pkg, ctx):
    """beamDetect's list is accepted and refined as the restatement refines its cells; the two lobes of one tone given by hand: in either order the first one is the
    representative and nu agrees between the orders; mergeTol = 0 keeps both; sidelobeMargin = 0 flags nothing."""
    r, s = _plain(pkg, ctx, "split273"), R.oracle_scene("split273")
    sc = r.sc
    est_mod = pkg.sensing.estimation
    c = pkg.Context()
    try:
        d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
        echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, r.rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c)
        est_mod.fft2D(r.rp, r.cf, echo, d_txg, ctx=c)
        bd = est_mod.beamDetect(c, est_mod.beamWeights(r.rp, [B.target_direction(sc, q)[0] for q in range(2)]))
        assert bd["row"].size >= 2
        st, raw = _raw(c, bd["row"], bd["col"])
        want = R.refine(s.rows_of(bd["row"]), bd["row"], bd["col"], s.n_fft, float(r.rp.vRes))
        print(f"beamDetect: rows {bd['row'].tolist()} cols {bd['col'].tolist()} -> parent {raw.parent.tolist()} sidelobe_of {raw.sidelobe_of.tolist()}; "
              f"margins {want.m2.min():.3e} {min(want.m4, default=np.inf):.3e} {min(want.m5, default=np.inf):.3e}")
        assert st == 0 and np.abs(raw.nu - want.nu).max() * s.L <= NU_TOL and np.array_equal(raw.status, want.status)
        if want.m2.min() >= 1e-6 and min(want.m4, default=1) >= 1e-6 and min(want.m5, default=1) >= 1e-6:   # (the conditioning of THIS list is not part of the CPU test)
            assert np.array_equal(raw.parent, want.parent) and np.array_equal(raw.sidelobe_of, want.sidelobe_of)
        d = est_mod.refineTargets(c, bd)
        assert d["n_in"] == bd["row"].size and d["row"].size == raw.n_kept and np.array_equal(d["rng"], bd["rng"][raw.parent == np.arange(raw.parent.size)])
        (r0, c0), (r1, c1) = R.SPLIT_LOBES
        st_a, a = _raw(c, [r0, r1], [c0, c1])
        st_b, b = _raw(c, [r1, r0], [c1, c0])
        assert st_a == st_b == 0 and a.parent.tolist() == b.parent.tolist() == [0, 0] and a.n_kept == b.n_kept == 1
        print(f"the two lobes: nu {a.nu.tolist()} / {b.nu.tolist()}; |difference| L {abs(a.nu[0] - a.nu[1]) * s.L:.3e}")
        assert np.abs(a.nu - b.nu[::-1]).max() * s.L <= NU_TOL and abs(a.nu[0] - b.nu[0]) * s.L <= NU_TOL
        assert a.nu.tobytes() == b.nu[::-1].tobytes()                          # an entry's values do not depend on its place in the input
        st0, z = _raw(c, [r0, r1], [c0, c1], merge_tol=0.0)
        assert st0 == 0 and z.n_kept == 2 and z.parent.tolist() == [0, 1]
        st1, f = _raw(c, r.tl["row"], r.tl["col"], margin=0.0)
        assert st1 == 0 and (f.sidelobe_of == -1).all() and np.array_equal(f.parent, r.raw.parent)
        d0 = est_mod.refineTargets(c, dict(row=[r0, r1], col=[c0, c1]), mergeTol=0)
        assert d0["row"].size == 2 and np.isnan(d0["rng"]).all()
    finally:
        c.close()


def test_existing_getters_are_untouched_by_the_call(pkg, ctx):
    """Detections, power window, covariance, MUSIC spectrum and the list itself byte-identical before and after; a pending submit and its result survive a (refused) call in
    between, and the collected CPI gives the refined list again."""
    r = _plain(pkg, ctx, "split273")
    for k in ("power_window", "Ra", "spectrum_db"):
        assert getattr(r.dbg, k).tobytes() == getattr(r.dbg_after, k).tobytes(), k
    assert (r.dbg.first_row, r.dbg.first_col) == (r.dbg_after.first_row, r.dbg_after.first_col)
    for a, b in zip(r.dbg.detections + r.dbg.det_pow, r.dbg_after.detections + r.dbg_after.det_pow):
        assert a.tobytes() == b.tobytes()
    for k in ("row", "col", "hits", "power", "rng", "vel", "azi", "snapshots"):
        assert r.tl[k].tobytes() == r.tl_after[k].tobytes(), k
    sc = r.sc
    F = import_module(pkg.__name__ + ".sensing.estimation.fft2D")
    d_txg, d_wave = ctx.to_device(sc.tx_grid), ctx.to_device(sc.tx_wave)
    echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, r.rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=ctx)
    F.fft2D_submit(r.rp, r.cf, echo, d_txg, ctx=ctx)
    with pytest.raises(pkg.IsacError) as e:                                 # submitted, not collected: no completed fft2D
        pkg.sensing.estimation.refineTargets(ctx, r.tl)
    assert e.value.name == "INVALID_ARG"
    est = F.fft2D_collect(ctx)
    for k in ("rngEst", "velEst", "aziEst"):
        assert getattr(est, k).tobytes() == getattr(r.est, k).tobytes(), k
    _same_out(pkg.sensing.estimation.refineTargets(ctx, pkg.sensing.estimation.targetList(ctx), snapshots=True), r.ref)


def test_call_on_one_context_leaves_another_contexts_pending_cpi_alone(pkg, ctx):
    """Two contexts on ONE pair of streams: c1 has a submitted, uncollected CPI (pending state, result in its pinned buffer) while c2 -- whose completed CPI sits behind it
    on the same streams -- refines its list; c1's collect then returns the very isac_est_result of the undisturbed run."""
    r = _plain(pkg, ctx, "split273")
    sc = r.sc
    F = import_module(pkg.__name__ + ".sensing.estimation.fft2D")
    c1, c2 = pkg.Context(), pkg.Context()
    try:
        c2.share_streams(c1)
        g1, w1, g2, w2 = c1.to_device(sc.tx_grid), c1.to_device(sc.tx_wave), c2.to_device(sc.tx_grid), c2.to_device(sc.tx_wave)
        e2 = pkg.sensing.monoStaticSensing(w2, sc.tx_grid.shape, sc.carrier, r.rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c2)
        pkg.sensing.estimation.fft2D(r.rp, r.cf, e2, g2, ctx=c2)
        e1 = pkg.sensing.monoStaticSensing(w1, sc.tx_grid.shape, sc.carrier, r.rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c1)
        F.fft2D_submit(r.rp, r.cf, e1, g1, ctx=c1)
        _same_out(pkg.sensing.estimation.refineTargets(c2, r.tl, snapshots=True), r.ref)
        res = pkg._lib.EstResult()
        c1.check(c1.lib.isac_fft2d_collect(c1.handle, C.byref(res)))
        ref = pkg._lib.EstResult()
        F.fft2D_submit(r.rp, r.cf, e1, g1, ctx=c1)
        c1.check(c1.lib.isac_fft2d_collect(c1.handle, C.byref(ref)))
        assert bytes(res) == bytes(ref)                                     # the whole isac_est_result, byte for byte
        _same_out(pkg.sensing.estimation.refineTargets(c1, r.tl, snapshots=True), r.ref)
    finally:
        c2.close()
        c1.close()


def test_contract(pkg):
    """ISAC_ERR_INVALID_ARG (1) before any fft2D, for n > ISAC_MAX_TARGETS, negative or NaN parameters, a cell outside the CUT zone, a UPA without ele, and after the range
    stage has rewritten the rows; n = 0 is ISAC_OK with n_kept = 0; a refused call leaves the CPI as it was."""
    L = pkg._lib
    s = R.oracle_scene("upa2x2_24prb")
    sc = s.sc
    rp, cf = _blocks(pkg, sc)
    est_mod = pkg.sensing.estimation
    c = pkg.Context()
    try:
        assert _raw(c, s.row, s.col)[0] == 1                               # before any fft2D
        assert _raw(c, [], [])[0] == 1                                     # ... also with n = 0: the context holds nothing
        d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
        echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c)
        with pytest.raises(pkg.IsacError) as e:                             # ISAC_OPT_UPA_DOA off: fft2D refuses its own DoA stage and has still collected the CPI
            est_mod.fft2D(rp, cf, echo, d_txg, ctx=c)
        assert e.value.name == "UNSUPPORTED"
        tl = est_mod.targetListUPA(c)
        st, full = _raw(c, tl["row"], tl["col"], A=sc.A)
        assert st == 0 and full.n_kept == s.ref.n_kept and np.array_equal(full.parent, s.ref.parent) and np.abs(full.nu - s.ref.nu).max() * s.L <= NU_TOL
        st, none = _raw(c, [], [])
        assert st == 0 and none.n_kept == 0                                # n = 0
        assert _raw(c, tl["row"], tl["col"], ele=False)[0] == 1            # a UPA without ele
        big = np.full(L.ISAC_MAX_TARGETS + 1, tl["row"][0], dtype=np.int32)
        assert _raw(c, big, np.full(big.size, tl["col"][0]))[0] == 1       # n > ISAC_MAX_TARGETS
        assert _raw(c, big[:-1], np.full(big.size - 1, tl["col"][0]))[0] == 0   # ... and ISAC_MAX_TARGETS itself is served
        assert _raw(c, tl["row"], tl["col"], n=-1)[0] == 1
        for kw in (dict(merge_tol=-1.0), dict(merge_tol=float("nan")), dict(merge_tol=float("inf")), dict(merge_rows=-1), dict(margin=-0.5), dict(margin=float("nan"))):
            assert _raw(c, tl["row"], tl["col"], **kw)[0] == 1, kw
        row0, row1, col0, col1 = s.rect
        for rr, cc in ((row0 - 1, col0), (row1 + 1, col0), (row0, col0 - 1), (row0, col1 + 1), (0, col0), (row0, 0)):
            assert _raw(c, [tl["row"][0], rr], [tl["col"][0], cc])[0] == 1, (rr, cc)   # outside the CUT zone
        for rr, cc in ((row0, col0), (row1, col1)):
            assert _raw(c, [rr], [cc])[0] == 0, (rr, cc)                   # its corners are inside
        with pytest.raises(pkg.IsacError) as e:
            est_mod.refineTargets(c, tl, mergeTol=-1)
        assert e.value.name == "INVALID_ARG"
        st, again = _raw(c, tl["row"], tl["col"], A=sc.A)                  # none of the refusals disturbed the CPI
        assert st == 0 and all(getattr(again, k).tobytes() == getattr(full, k).tobytes() for k in ("status", "parent", "sidelobe_of", "nu", "vel", "power", "azi", "ele", "snapshots"))
        c.set_upa_doa(True)                                                 # ISAC_OPT_UPA_DOA on: the same answer
        est_mod.fft2D(rp, cf, echo, d_txg, ctx=c)
        st, on = _raw(c, tl["row"], tl["col"], A=sc.A)
        assert st == 0 and all(getattr(on, k).tobytes() == getattr(full, k).tobytes() for k in ("status", "parent", "sidelobe_of", "nu", "vel", "power", "azi", "ele", "snapshots"))
        # the range stage alone on OTHER grids rewrites the range rows: no stale answer
        im = import_module
        ep, cfb = im(pkg.__name__ + ".sensing._marshal").est_block(rp), im(pkg.__name__ + ".sensing.estimation.fft2D")._cfar_block(cf)
        other = c.to_device(np.asfortranarray(sc.tx_grid[:, ::-1, :]))
        c.check(c.lib.isac_fft2d_range_stage_dev(c.handle, C.byref(ep), C.byref(cfb), other, d_txg, sc.K, sc.L, sc.A))
        assert _raw(c, tl["row"], tl["col"])[0] == 1
    finally:
        c.close()
