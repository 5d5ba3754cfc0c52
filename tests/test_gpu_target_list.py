"""isac_fft2d_get_targets on the MI355X: the per-target list of fft2D (paired range, velocity, azimuth; project-defined -- include/isac_targets.h).

Scenes and the oracle-only result come from tests/_target_list_restatement.py; tests/test_target_list_cpu.py has shown on the oracle that every decision of every target
in them clears the 1e-9 guard band, so nothing here is left out or skipped.  The 273-PRB scenes have L = 56 symbols (four slots), not 28: at 28 symbols zero-padded to
nFFT = 256 the CA-CFAR training cells lie inside the Doppler main lobe and fft2D detects nothing (the restatement module says why in full).
The single-target check "Bartlett azimuth == fft2D's aziEst[0]" is not made: on the oracle the two differ (fft2D forms Ra from the conjugate-transposed grid, fft2D.m:106-107,
one-way, while the snapshot of a cell carries the two-way phase of the path "transmit element a -> receive element a": tests/test_target_list_cpu.py records the figures
and the relation sind(azi) = -2 sind(aziEst)); a check the oracle does not bear out is not made on the device either."""
from __future__ import annotations

import ctypes as C
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest

import oracle as O
from conftest import make_scene
from oracle.music import ula_scan_angles

import _target_list_restatement as R

pytestmark = pytest.mark.gpu

LIST_KEYS = ("row", "col", "hits", "power", "rng", "vel", "azi")


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context()
    yield c
    c.close()


def _same_list(a, b):
    assert a["n_total"] == b["n_total"]
    for k in LIST_KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k


def _blocks(pkg, sc):
    rp = pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)
    return rp, pkg.sensing.detection.cfar2D(rp)


_runs = {}


def _plain(pkg, ctx, name):
    """Scene `name` through monoStaticSensing -> plain isac_fft2d_dev -> the getters -> isac_fft2d_get_targets, once per module (host copies only)."""
    if name not in _runs:
        sc = R.make(name)
        rp, cf = _blocks(pkg, sc)
        cf = R.with_bands(name, cf)                                          # the default bands for every scene but R.BAND_SCENE
        d_txg, d_wave = ctx.to_device(sc.tx_grid), ctx.to_device(sc.tx_wave)
        echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=ctx)
        est, dbg = pkg.sensing.estimation.fft2D(rp, cf, echo, d_txg, return_debug=True, ctx=ctx)
        if name == R.BAND_SCENE:
            (gr, gc), (tr, tc) = R.bands_of(name)
            assert dbg.power_window.shape[:2] == (cf.CUTIdx[0].max() - cf.CUTIdx[0].min() + 1 + 2 * (gr + tr), cf.CUTIdx[1].max() - cf.CUTIdx[1].min() + 1 + 2 * (gc + tc))
        tl = pkg.sensing.estimation.targetList(ctx, snapshots=True)
        dbg2 = import_module(pkg.__name__ + ".sensing.estimation.fft2D").fft2D_debug(ctx, sc.A)
        for d in (echo, d_txg, d_wave):
            d.free()
        from_cf = import_module(pkg.__name__ + ".sensing.estimation.fft2D")._cut_rectangle(cf.CUTIdx)
        _runs[name] = SimpleNamespace(sc=sc, rp=rp, cf=cf, est=est, dbg=dbg, dbg_after=dbg2, tl=tl, rect=from_cf)
    return _runs[name]


@pytest.mark.parametrize("name", list(R.SCENES))
def test_cells_equal_the_restatement_on_the_devices_own_window(pkg, ctx, name):
    """Kernel level, exact: steps 1, 2 and 5 of the restatement on the device's own power window and detection lists."""
    r = _plain(pkg, ctx, name)
    want = R.target_cells(r.dbg.power_window, r.dbg.detections, r.dbg.first_row, r.dbg.first_col, r.rect, int(r.rp.nIFFT))
    print(f"{name}: {r.tl['n_total']} targets, rows {r.tl['row'][:6].tolist()} cols {r.tl['col'][:6].tolist()} azi {r.tl['azi'][:6].tolist()}")
    assert r.tl["n_total"] == want.row.size >= 1
    assert np.array_equal(r.tl["row"], want.row) and np.array_equal(r.tl["col"], want.col) and np.array_equal(r.tl["hits"], want.hits)
    assert r.tl["power"].tobytes() == want.power.tobytes()
    assert np.array_equal(r.tl["rng"], (want.row - 1) * r.rp.rRes) and np.array_equal(r.tl["vel"], (want.col - int(r.rp.nFFT) / 2 - 1) * r.rp.vRes)


@pytest.mark.parametrize("name", list(R.SCENES))
def test_snapshots_and_azimuth(pkg, ctx, name):
    """x against the oracle's rdm at the target cells to 1e-10 of max |rdm| (the project's field tolerance); azi = the restatement's arg-max on the DEVICE's snapshots,
    and always the lowest scan index among the angles with the same sind (the lower mirror twin)."""
    r, t = _plain(pkg, ctx, name), R.oracle_targets(name)
    x = r.tl["snapshots"]
    err = np.abs(x - t.rdm_at(r.tl["row"], r.tl["col"])).max() / t.rdm_max
    bins, azi, margin2, _ = R.bartlett(x, r.rp)
    print(f"{name}: snapshot error {err:.3e} of max |rdm|; min margin2 on the device's snapshots {margin2.min():.3e}")
    assert err <= 1e-10
    assert np.array_equal(r.tl["azi"], azi)
    sd = np.array([float(O.sind(a)) for a in ula_scan_angles(r.rp)])
    assert all(int(b) == int(np.flatnonzero(sd == sd[b])[0]) for b in bins)


@pytest.mark.parametrize("name", list(R.SCENES))
def test_chain_equals_the_oracle_only_result(pkg, ctx, name):
    r, t = _plain(pkg, ctx, name), R.oracle_targets(name)
    tl = r.tl
    assert tl["n_total"] == t.row.size
    assert np.array_equal(tl["row"], t.row) and np.array_equal(tl["col"], t.col) and np.array_equal(tl["hits"], t.hits)
    assert np.array_equal(tl["azi"], t.azi) and np.array_equal(tl["rng"], t.rng) and np.array_equal(tl["vel"], t.vel)
    rel = np.abs(tl["power"] - t.power).max() / t.power.max()
    print(f"{name}: power error {np.abs(tl['power'] / t.power - 1).max():.3e} relative")
    assert (np.abs(tl["power"] - t.power) <= 1e-10 * t.power).all(), rel


def test_existing_getters_are_untouched_by_the_call(pkg, ctx):
    """Detections, power window, covariance and MUSIC spectrum byte-identical before and after; a pending submit and its result survive a (refused) call in between."""
    r = _plain(pkg, ctx, "a4_273prb")
    for k in ("power_window", "Ra", "spectrum_db"):
        assert getattr(r.dbg, k).tobytes() == getattr(r.dbg_after, k).tobytes(), k
    assert (r.dbg.first_row, r.dbg.first_col) == (r.dbg_after.first_row, r.dbg_after.first_col)
    for a, b in zip(r.dbg.detections + r.dbg.det_pow, r.dbg_after.detections + r.dbg_after.det_pow):
        assert a.tobytes() == b.tobytes()
    sc = r.sc
    F = import_module(pkg.__name__ + ".sensing.estimation.fft2D")
    d_txg, d_wave = ctx.to_device(sc.tx_grid), ctx.to_device(sc.tx_wave)
    echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, r.rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=ctx)
    F.fft2D_submit(r.rp, r.cf, echo, d_txg, ctx=ctx)
    with pytest.raises(pkg.IsacError) as e:                                 # submitted, not collected: no completed fft2D
        pkg.sensing.estimation.targetList(ctx)
    assert e.value.name == "INVALID_ARG"
    est = F.fft2D_collect(ctx)
    for k in ("rngEst", "velEst", "aziEst"):
        assert getattr(est, k).tobytes() == getattr(r.est, k).tobytes(), k
    _same_list(pkg.sensing.estimation.targetList(ctx), r.tl)              # and the collected CPI gives the list again


def test_routes_give_the_same_list(pkg, ctx):
    """Plain isac_fft2d_dev == fused + cached with a caller's echo grid == ISAC_OPT_TAIL_FUSION 0 / 1 x ISAC_OPT_WIDE_ORDER 0 / 1, bit for bit."""
    r = _plain(pkg, ctx, "a4_273prb")
    sc = r.sc
    c2 = pkg.Context()
    try:
        d_txg, d_wave = c2.to_device(sc.tx_grid), c2.to_device(sc.tx_wave)
        echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, r.rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, fuse_fft2d=(r.rp, r.cf, d_txg), ctx=c2)
        pkg.sensing.estimation.fft2D(r.rp, r.cf, echo, d_txg, reuse_range=True, ctx=c2)
        _same_list(pkg.sensing.estimation.targetList(c2), r.tl)
        for tail in (False, True):
            for wide in (True, False):
                c2.set_tail_fusion(tail)
                c2.set_wide_order(wide)
                pkg.sensing.estimation.fft2D(r.rp, r.cf, echo, d_txg, ctx=c2)
                _same_list(pkg.sensing.estimation.targetList(c2), r.tl)
    finally:
        c2.close()


def test_lazy_grid_gives_the_same_list(pkg):
    """A = 64, Q = 1, Philox spectral noise, L = 28 (~100 MB): the echo grid the context re-forms (never stored) against the stored one.  nFFT = 64 so that the
    28-symbol scene has detections at all."""
    sc = make_scene(n_ants=64, n_slots=2, num_slots_param=6, with_noise=False, zero_s_slots=False, seed=31)
    rp, cf = _blocks(pkg, sc)
    c = pkg.Context()
    try:
        d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
        kw = dict(nfft=4096, fuse_fft2d=(rp, cf, d_txg), ctx=c, seed=77, noise_domain="spectral")
        arr = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, **kw)
        pkg.sensing.estimation.fft2D(rp, cf, arr, d_txg, reuse_range=True, ctx=c)
        stored = pkg.sensing.estimation.targetList(c, snapshots=True)
        lz = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, lazy=True, **kw)
        pkg.sensing.estimation.fft2D(rp, cf, lz, d_txg, reuse_range=True, ctx=c)
        lazy = pkg.sensing.estimation.targetList(c, snapshots=True)
        assert stored["n_total"] >= 1 and stored["hits"].max() == 64
        _same_list(lazy, stored)
        assert lazy["snapshots"].tobytes() == stored["snapshots"].tobytes()
    finally:
        c.close()


def test_submit_n_each_context_returns_its_own_list(pkg):
    """Two jobs through isac_sensing_submit_n / collect_n: each context's list is the one its own job gives through the single calls."""
    sc = R.make("a4_273prb")
    rp, cf = _blocks(pkg, sc)
    ctxs = [pkg.Context() for _ in range(3)]
    try:
        seeds = [101, 202]
        waves = [c.to_device(sc.tx_wave) for c in ctxs]
        grids = [c.to_device(sc.tx_grid) for c in ctxs]
        single = []
        for s in seeds:
            echo = pkg.sensing.monoStaticSensing(waves[2], sc.tx_grid.shape, sc.carrier, rp, sc.los, nfft=4096, fuse_fft2d=(rp, cf, grids[2]), ctx=ctxs[2], seed=s,
                                                 noise_domain="spectral")
            pkg.sensing.estimation.fft2D(rp, cf, echo, grids[2], reuse_range=True, ctx=ctxs[2])
            single.append(pkg.sensing.estimation.targetList(ctxs[2]))
        echoes = [c.empty(sc.tx_grid.shape) for c in ctxs[:2]]
        batch = pkg.sensing.submitN(ctxs[:2], waves[:2], grids[:2], sc.tx_grid.shape, sc.carrier, [rp, rp], [sc.los, sc.los], cf, seeds=seeds, nfft=4096, echoGrids=echoes)
        res = batch.collect()
        assert not any(isinstance(x, Exception) for x in res)
        for c, want in zip(ctxs[:2], single):
            _same_list(pkg.sensing.estimation.targetList(c), want)
        assert single[0]["n_total"] >= 2 and single[0]["power"].tobytes() != single[1]["power"].tobytes()      # two different noise fields: two different lists
    finally:
        for c in ctxs:
            c.close()


def test_contract(pkg):
    L = pkg._lib
    sc = R.make("a4_24prb_generic")
    rp, cf = _blocks(pkg, sc)
    c = pkg.Context()
    try:
        with pytest.raises(pkg.IsacError) as e:                             # before any fft2D
            pkg.sensing.estimation.targetList(c)
        assert e.value.name == "INVALID_ARG"
        d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
        echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c)
        pkg.sensing.estimation.fft2D(rp, cf, echo, d_txg, ctx=c)
        full = pkg.sensing.estimation.targetList(c)
        assert full["n_total"] >= 2
        out = L.TargetList()
        snap = np.zeros((sc.A, 1), dtype=np.complex128, order="F")
        assert c.lib.isac_fft2d_get_targets(c.handle, C.byref(out), snap.ctypes.data_as(C.c_void_p), 1) == 6      # ISAC_ERR_CAPACITY: fewer snapshot columns than targets
        assert out.n_total == full["n_total"]
        assert c.lib.isac_fft2d_get_targets(c.handle, C.byref(out), None, 0) == 0 and out.n_targets == full["n_total"]   # without snapshots the capacity does not matter
        # the range stage alone on OTHER grids rewrites the range rows: no stale answer
        im = import_module
        ep, cfb = im(pkg.__name__ + ".sensing._marshal").est_block(rp), im(pkg.__name__ + ".sensing.estimation.fft2D")._cfar_block(cf)
        other = c.to_device(np.asfortranarray(sc.tx_grid[:, ::-1, :]))
        c.check(c.lib.isac_fft2d_range_stage_dev(c.handle, C.byref(ep), C.byref(cfb), other, d_txg, sc.K, sc.L, sc.A))
        with pytest.raises(pkg.IsacError) as e:
            pkg.sensing.estimation.targetList(c)
        assert e.value.name == "INVALID_ARG"
        # a UPA: fft2D itself refuses the DoA (range and velocity are reported), and so does the target list, whatever ISAC_OPT_UPA_DOA says
        rp_upa = SimpleNamespace(**vars(rp))
        rp_upa.antennaType = SimpleNamespace(kind="upa", nV=2, nH=2)
        for on in (False, True):
            c.set_upa_doa(on)
            try:
                pkg.sensing.estimation.fft2D(rp_upa, cf, echo, d_txg, ctx=c)
                assert on
            except pkg.IsacError as err:
                assert on or err.name == "UNSUPPORTED"
            with pytest.raises(pkg.IsacError) as e:
                pkg.sensing.estimation.targetList(c)
            assert e.value.name == "UNSUPPORTED"
    finally:
        c.close()


def test_call_on_one_context_leaves_another_contexts_pending_cpi_alone(pkg, ctx):
    """Two contexts on ONE pair of streams: c1 has a submitted, uncollected CPI (pending state, result in its pinned buffer) while c2 -- whose completed CPI sits behind it
    on the same streams -- produces its list; c1's collect then returns the very isac_est_result of the undisturbed run, and c2's list is the reference list."""
    r = _plain(pkg, ctx, "a4_273prb")
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
        _same_list(pkg.sensing.estimation.targetList(c2), r.tl)
        res = pkg._lib.EstResult()
        c1.check(c1.lib.isac_fft2d_collect(c1.handle, C.byref(res)))
        ref = pkg._lib.EstResult()
        F.fft2D_submit(r.rp, r.cf, e1, g1, ctx=c1)
        c1.check(c1.lib.isac_fft2d_collect(c1.handle, C.byref(ref)))
        assert bytes(res) == bytes(ref)                                     # the whole isac_est_result, byte for byte
        assert np.array_equal(np.array(res.rng_est[: res.n_rng]), r.est.rngEst) and np.array_equal(np.array(res.azi_est[: res.n_azi]), r.est.aziEst)
        _same_list(pkg.sensing.estimation.targetList(c1), r.tl)
    finally:
        c2.close()
        c1.close()


def test_mex_command_equals_the_c_call(pkg, ctx, tmp_path):
    """'fft2DTargets' through mexFunction (tests/mex_targets_host.cpp, the way mex/matlab/+sensing/+estimation/targetList.m calls it), after 'fft2D' on MATLAB arrays:
    an [n x 1] struct array whose fields equal isac_fft2d_get_targets' list of the same scene, bit for bit; before any fft2D the command raises isac:INVALID_ARG."""
    import struct
    import subprocess
    import __graft_entry__ as g
    exe = g.build_mex_targets_host()
    r = _plain(pkg, ctx, "a4_24prb_generic")
    sc, rp = r.sc, r.rp
    echo = pkg.sensing.monoStaticSensing(sc.tx_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=ctx)
    row0, row1, col0, col1 = r.rect
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<14i 5d", sc.K, sc.L, sc.A, int(rp.nIFFT), int(rp.nFFT), 2, 2, 1, 1, row0, row1, col0, col1, 0, float(rp.rRes), float(rp.vRes), float(rp.Pfa),
                            float(rp.azimuthScanScale), float(rp.azimuthScanGranularity)))
        f.write(np.asfortranarray(echo).tobytes(order="F"))
        f.write(np.asfortranarray(sc.tx_grid).tobytes(order="F"))
    p = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    assert p.stdout.split() == ["isac:INVALID_ARG"]
    raw = open(fout, "rb").read()
    n = struct.unpack_from("<i", raw)[0]
    vals = np.frombuffer(raw, dtype=np.float64, offset=4).reshape(7, n)
    assert n == r.tl["n_total"] >= 2
    for k, v in zip(("rng", "vel", "azi", "power", "hits", "row", "col"), vals):
        assert v.tobytes() == r.tl[k].astype(np.float64).tobytes(), k
