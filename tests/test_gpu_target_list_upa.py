"""isac_fft2d_get_targets_upa on the MI355X: the per-target list of fft2D for a uniform planar array (paired range, velocity, azimuth, elevation; project-defined --
include/isac_targets_upa.h).

Scenes and the oracle-only result come from tests/_target_list_upa_restatement.py; tests/test_target_list_upa_cpu.py has shown on the oracle that every decision of every
target in them clears the 1e-9 guard band, so nothing here is left out or skipped.  Each scene runs once per module."""
from __future__ import annotations

import ctypes as C
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import make_scene

import _target_list_restatement as T
import _target_list_upa_restatement as R

pytestmark = pytest.mark.gpu

CELL_KEYS = ("row", "col", "hits", "power", "rng", "vel")
LIST_KEYS = CELL_KEYS + ("azi", "ele")


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context()
    c.set_upa_doa(True)
    yield c
    c.close()


def _same_list(a, b, keys=LIST_KEYS):
    assert a["n_total"] == b["n_total"]
    for k in keys:
        assert a[k].tobytes() == b[k].tobytes(), k


def _blocks(pkg, sc):
    rp = pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)
    return rp, pkg.sensing.detection.cfar2D(rp)


def _as_ula(rp, n_ants):
    r = SimpleNamespace(**vars(rp))
    r.antennaType = SimpleNamespace(kind="ula", numElements=n_ants, d=0.5)
    return r


_runs = {}


def _plain(pkg, ctx, name):
    """Scene `name` through monoStaticSensing -> isac_fft2d_dev (ISAC_OPT_UPA_DOA on) -> the getters -> isac_fft2d_get_targets_upa -> the getters again, then the SAME echo
    grid through fft2D with the array declared a ULA -> isac_fft2d_get_targets.  Once per module (host copies only)."""
    if name not in _runs:
        sc = R.make(name)
        rp, cf = _blocks(pkg, sc)
        cf = T.with_bands(name, cf)                                          # the default bands for every scene but R.BAND_SCENE
        est_mod = pkg.sensing.estimation
        d_txg, d_wave = ctx.to_device(sc.tx_grid), ctx.to_device(sc.tx_wave)
        echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=ctx)
        est, dbg = est_mod.fft2D(rp, cf, echo, d_txg, return_debug=True, ctx=ctx)
        if name == R.BAND_SCENE:
            (gr, gc), (tr, tc) = T.bands_of(name)
            assert (gr + tr, gc + tc) == (4, 5) and dbg.power_window.shape[:2] == (np.ptp(cf.CUTIdx[0]) + 1 + 2 * (gr + tr), np.ptp(cf.CUTIdx[1]) + 1 + 2 * (gc + tc))
        tl = est_mod.targetListUPA(ctx, snapshots=True)
        map_after = ctx.angular_spectrum2d()
        with pytest.raises(pkg.IsacError) as e:                              # the ULA entry point keeps refusing a UPA
            est_mod.targetList(ctx)
        assert e.value.name == "UNSUPPORTED"
        est_mod.fft2D(_as_ula(rp, sc.A), cf, echo, d_txg, ctx=ctx)
        ula = est_mod.targetList(ctx, snapshots=True)
        for d in (echo, d_txg, d_wave):
            d.free()
        rect = import_module(pkg.__name__ + ".sensing.estimation.fft2D")._cut_rectangle(cf.CUTIdx)
        _runs[name] = SimpleNamespace(sc=sc, rp=rp, cf=cf, est=est, dbg=dbg, map_after=map_after, tl=tl, ula=ula, rect=rect)
    return _runs[name]


@pytest.mark.parametrize("name", list(R.SCENES))
def test_cells_equal_the_restatement_on_the_devices_own_window(pkg, ctx, name):
    """Kernel level, exact: steps 1, 2 and 5 of the restatement on the device's own power window and detection lists."""
    r = _plain(pkg, ctx, name)
    want = T.target_cells(r.dbg.power_window, r.dbg.detections, r.dbg.first_row, r.dbg.first_col, r.rect, int(r.rp.nIFFT))
    tl = r.tl
    print(f"{name}: {tl['n_total']} targets, rows {tl['row'][:6].tolist()} cols {tl['col'][:6].tolist()} azi {tl['azi'][:6].tolist()} ele {tl['ele'][:6].tolist()}")
    assert tl["n_total"] == want.row.size >= 1
    assert np.array_equal(tl["row"], want.row) and np.array_equal(tl["col"], want.col) and np.array_equal(tl["hits"], want.hits)
    assert tl["power"].tobytes() == want.power.tobytes()
    assert np.array_equal(tl["rng"], (want.row - 1) * r.rp.rRes) and np.array_equal(tl["vel"], (want.col - int(r.rp.nFFT) / 2 - 1) * r.rp.vRes)


@pytest.mark.parametrize("name", list(R.SCENES))
def test_same_bits_as_the_ula_entry(pkg, ctx, name):
    """Steps 1, 2, 3 and 5 do not know the array type: the same echo grid through fft2D as a ULA and isac_fft2d_get_targets gives the same cells, powers, ranges,
    velocities, count and snapshots, byte for byte."""
    r = _plain(pkg, ctx, name)
    _same_list(r.ula, r.tl, CELL_KEYS)
    assert r.ula["snapshots"].tobytes() == r.tl["snapshots"].tobytes()
    assert "ele" not in r.ula and r.tl["ele"].shape == r.tl["azi"].shape


@pytest.mark.parametrize("name", list(R.SCENES))
def test_snapshots_and_angles(pkg, ctx, name):
    """x against the oracle's rdm at the target cells to 1e-10 of max |rdm| (the project's field tolerance); (azi, ele) = the restatement's arg-max on the DEVICE's
    snapshots, exactly, and always the lowest grid index among the points that carry the same steering vector (the lower mirror twin)."""
    r, t = _plain(pkg, ctx, name), R.oracle_targets(name)
    x = r.tl["snapshots"]
    err = np.abs(x - t.rdm_at(r.tl["row"], r.tl["col"])).max() / t.rdm_max
    js, azi, ele, margin2, ties = R.bartlett2d(x, r.sc.nV, r.sc.nH, r.rp)
    print(f"{name}: snapshot error {err:.3e} of max |rdm|; min margin2 on the device's snapshots {margin2.min():.3e}; ties {ties.tolist()}")
    assert err <= 1e-10
    assert np.array_equal(r.tl["azi"], azi) and np.array_equal(r.tl["ele"], ele)
    e_steps = int(np.floor((r.rp.elevationScanScale + 1) / r.rp.elevationScanGranularity))
    dev_j = np.rint((r.tl["ele"] + r.rp.elevationScanScale / 2.0) / r.rp.elevationScanGranularity).astype(int) + e_steps * np.rint(
        (r.tl["azi"] + r.rp.azimuthScanScale / 2.0) / r.rp.azimuthScanGranularity).astype(int)
    assert np.array_equal(dev_j, js)
    assert all(int(j) == R.lowest_equal(j, r.sc.nV, r.sc.nH, r.rp) for j in dev_j)


@pytest.mark.parametrize("name", list(R.SCENES))
def test_chain_equals_the_oracle_only_result(pkg, ctx, name):
    r, t = _plain(pkg, ctx, name), R.oracle_targets(name)
    tl = r.tl
    assert tl["n_total"] == t.row.size
    assert np.array_equal(tl["row"], t.row) and np.array_equal(tl["col"], t.col) and np.array_equal(tl["hits"], t.hits)
    assert np.array_equal(tl["azi"], t.azi) and np.array_equal(tl["ele"], t.ele) and np.array_equal(tl["rng"], t.rng) and np.array_equal(tl["vel"], t.vel)
    print(f"{name}: power error {np.abs(tl['power'] / t.power - 1).max():.3e} relative")
    assert (np.abs(tl["power"] - t.power) <= 1e-10 * t.power).all()


def test_the_list_does_not_depend_on_the_upa_doa_option(pkg, ctx):
    """ISAC_OPT_UPA_DOA off: fft2D raises UNSUPPORTED for its own DoA stage and the list is returned all the same; on: the same list, byte for byte, and fft2D's own
    estimates and its dB map are byte-identical before and after the call."""
    r = _plain(pkg, ctx, "upa2x4_24prb")
    sc = r.sc
    est_mod = pkg.sensing.estimation
    assert r.dbg.spectrum_db_2d.tobytes() == r.map_after.tobytes()          # the map of the first run, read before and after the list
    c = pkg.Context()
    try:
        d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
        echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, r.rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c)
        with pytest.raises(pkg.IsacError) as e:
            est_mod.fft2D(r.rp, r.cf, echo, d_txg, ctx=c)
        assert e.value.name == "UNSUPPORTED"
        off = est_mod.targetListUPA(c, snapshots=True)
        _same_list(off, r.tl)
        assert off["snapshots"].tobytes() == r.tl["snapshots"].tobytes()
        c.set_upa_doa(True)
        est, dbg = est_mod.fft2D(r.rp, r.cf, echo, d_txg, return_debug=True, ctx=c)
        on = est_mod.targetListUPA(c, snapshots=True)
        _same_list(on, r.tl)
        assert on["snapshots"].tobytes() == r.tl["snapshots"].tobytes()
        assert c.angular_spectrum2d().tobytes() == dbg.spectrum_db_2d.tobytes() == r.dbg.spectrum_db_2d.tobytes()
        for k in ("rngEst", "velEst", "aziEst", "eleEst"):
            assert getattr(est, k).tobytes() == getattr(r.est, k).tobytes(), k
        assert np.all(np.isfinite(est.eleEst))
    finally:
        c.close()


def test_lazy_grid_gives_the_same_list(pkg):
    """8 x 8, A = 64, Q = 1, Philox spectral noise, L = 28 (~100 MB): the echo grid the context re-forms (never stored) against the stored one.  nFFT = 64 so that the
    28-symbol scene has detections at all."""
    sc = make_scene(n_ants=64, n_slots=2, num_slots_param=6, with_noise=False, zero_s_slots=False, seed=31)
    sc.cell.gNBSenAntenna = SimpleNamespace(kind="upa", nV=8, nH=8, dV=0.5, dH=0.5)
    rp, cf = _blocks(pkg, sc)
    c = pkg.Context()
    c.set_upa_doa(True)
    try:
        d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
        kw = dict(nfft=4096, fuse_fft2d=(rp, cf, d_txg), ctx=c, seed=77, noise_domain="spectral")
        arr = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, **kw)
        pkg.sensing.estimation.fft2D(rp, cf, arr, d_txg, reuse_range=True, ctx=c)
        stored = pkg.sensing.estimation.targetListUPA(c, snapshots=True)
        lz = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, lazy=True, **kw)
        pkg.sensing.estimation.fft2D(rp, cf, lz, d_txg, reuse_range=True, ctx=c)
        lazy = pkg.sensing.estimation.targetListUPA(c, snapshots=True)
        assert stored["n_total"] >= 1 and stored["hits"].max() == 64
        _same_list(lazy, stored)
        assert lazy["snapshots"].tobytes() == stored["snapshots"].tobytes()
    finally:
        c.close()


def test_contract(pkg):
    L = pkg._lib
    sc = R.make("upa2x2_24prb")
    rp, cf = _blocks(pkg, sc)
    est_mod = pkg.sensing.estimation
    c = pkg.Context()
    try:
        with pytest.raises(pkg.IsacError) as e:                             # before any fft2D
            est_mod.targetListUPA(c)
        assert e.value.name == "INVALID_ARG"
        d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
        echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c)
        # a ULA context: the other entry point's list
        est_mod.fft2D(_as_ula(rp, sc.A), cf, echo, d_txg, ctx=c)
        with pytest.raises(pkg.IsacError) as e:
            est_mod.targetListUPA(c)
        assert e.value.name == "UNSUPPORTED" and "isac_fft2d_get_targets" in str(e.value)
        # nV x nH is not the antenna count (option off: fft2D reports its DoA stage as unsupported and has still collected the CPI)
        rp_bad = SimpleNamespace(**vars(rp))
        rp_bad.antennaType = SimpleNamespace(kind="upa", nV=2, nH=3)
        with pytest.raises(pkg.IsacError) as e:
            est_mod.fft2D(rp_bad, cf, echo, d_txg, ctx=c)
        assert e.value.name == "UNSUPPORTED"
        with pytest.raises(pkg.IsacError) as e:
            est_mod.targetListUPA(c)
        assert e.value.name == "INVALID_ARG"
        # the scene itself
        with pytest.raises(pkg.IsacError) as e:
            est_mod.fft2D(rp, cf, echo, d_txg, ctx=c)
        assert e.value.name == "UNSUPPORTED"
        full = est_mod.targetListUPA(c)
        assert full["n_total"] >= 2
        out = L.TargetList()
        ele = (C.c_double * L.ISAC_MAX_TARGETS)()
        snap = np.zeros((sc.A, 1), dtype=np.complex128, order="F")
        assert c.lib.isac_fft2d_get_targets_upa(c.handle, C.byref(out), None, None, 0) == 1                           # ele == NULL: ISAC_ERR_INVALID_ARG
        assert c.lib.isac_fft2d_get_targets_upa(c.handle, None, ele, None, 0) == 1
        assert c.lib.isac_fft2d_get_targets_upa(c.handle, C.byref(out), ele, snap.ctypes.data_as(C.c_void_p), 1) == 6   # ISAC_ERR_CAPACITY: fewer snapshot columns than targets
        assert out.n_total == full["n_total"]
        assert c.lib.isac_fft2d_get_targets_upa(c.handle, C.byref(out), ele, None, 0) == 0 and out.n_targets == full["n_total"]   # without snapshots the capacity does not matter
        assert np.array_equal(np.array(ele[: out.n_targets]), full["ele"])
        with pytest.raises(pkg.IsacError) as e:                             # the ULA entry point on the same UPA context: refused as before
            est_mod.targetList(c)
        assert e.value.name == "UNSUPPORTED"
        # the range stage alone on OTHER grids rewrites the range rows: no stale answer
        im = import_module
        ep, cfb = im(pkg.__name__ + ".sensing._marshal").est_block(rp), im(pkg.__name__ + ".sensing.estimation.fft2D")._cfar_block(cf)
        other = c.to_device(np.asfortranarray(sc.tx_grid[:, ::-1, :]))
        c.check(c.lib.isac_fft2d_range_stage_dev(c.handle, C.byref(ep), C.byref(cfb), other, d_txg, sc.K, sc.L, sc.A))
        with pytest.raises(pkg.IsacError) as e:
            est_mod.targetListUPA(c)
        assert e.value.name == "INVALID_ARG"
    finally:
        c.close()


def test_call_on_one_context_leaves_another_contexts_pending_cpi_alone(pkg, ctx):
    """Two contexts on ONE pair of streams: c1 has a submitted, uncollected CPI (pending state, result in its pinned buffer) while c2 -- whose completed CPI sits behind it
    on the same streams -- produces its list; c1's collect then returns the very isac_est_result of the undisturbed run, and c2's list is the reference list."""
    r = _plain(pkg, ctx, "upa2x4_24prb")
    sc = r.sc
    F = import_module(pkg.__name__ + ".sensing.estimation.fft2D")
    c1, c2 = pkg.Context(), pkg.Context()
    try:
        c1.set_upa_doa(True)
        c2.set_upa_doa(True)
        c2.share_streams(c1)
        g1, w1, g2, w2 = c1.to_device(sc.tx_grid), c1.to_device(sc.tx_wave), c2.to_device(sc.tx_grid), c2.to_device(sc.tx_wave)
        e2 = pkg.sensing.monoStaticSensing(w2, sc.tx_grid.shape, sc.carrier, r.rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c2)
        pkg.sensing.estimation.fft2D(r.rp, r.cf, e2, g2, ctx=c2)
        e1 = pkg.sensing.monoStaticSensing(w1, sc.tx_grid.shape, sc.carrier, r.rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c1)
        F.fft2D_submit(r.rp, r.cf, e1, g1, ctx=c1)
        _same_list(pkg.sensing.estimation.targetListUPA(c2), r.tl)
        res = pkg._lib.EstResult()
        c1.check(c1.lib.isac_fft2d_collect(c1.handle, C.byref(res)))
        ref = pkg._lib.EstResult()
        F.fft2D_submit(r.rp, r.cf, e1, g1, ctx=c1)
        c1.check(c1.lib.isac_fft2d_collect(c1.handle, C.byref(ref)))
        assert bytes(res) == bytes(ref)                                     # the whole isac_est_result, byte for byte
        assert np.array_equal(np.array(res.rng_est[: res.n_rng]), r.est.rngEst) and np.array_equal(np.array(res.ele_est[: res.n_azi]), r.est.eleEst)
        _same_list(pkg.sensing.estimation.targetListUPA(c1), r.tl)
    finally:
        c2.close()
        c1.close()
