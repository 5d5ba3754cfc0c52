"""music_scan_kernel's three ULA spectra (csrc/music.hip: MUSIC on both eigensolver routes, digitalBF, mvdrBF) value by value: the device's dB spectrum,
read through Context.angular_spectrum(), against the extended-precision reference of tests/_doa_reference.py at TOL_DB = 1e-6 dB per scan point (the
tolerance of the UPA maps, tests/test_gpu_upa_doa.py); where the reference lies above -200 dB both sides must be finite.  The estimate lists of
isac_music_doa / isac_beamscan_doa must equal findpeaks on the DEVICE'S OWN spectrum, which separates the kernel from the host tail.

* array sizes by dispatch boundary (_doa_reference.ARRAY_SIZES), eigenvalue spreads 1e1 / 1e4 / 1e7, MUSIC's numDets from 1 to past the array size on
  set_music_route(0) and (1), each against the reference;
* physical sample covariances against mpmath, one of them with three different peak lists for the three methods;
* two non-default scan grids on one context after the default one (the cached sine table);
* the fft2D chain at A = 8 (mpmath on the device's Ra) and A = 65 (sign-function projector);
* the contract of isac_fft2d_get_music_spectrum (include/isac.h).

tests/test_doa_spectra_cpu.py holds the inputs' conditions (the fp64 formulations within 1e-8 dB of the reference on every case here) and shows that
this comparison rejects a swapped DBF / MVDR weight, a MUSIC with L +- 1, fp32 steering phases, d off by 1e-7, the opposite phase sign, a mean
normalisation and a scan shifted by one step.  Largest deviations measured on an MI355X: DESIGN.md section 5."""
from __future__ import annotations

import copy
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest

import _doa_reference as R
import oracle as O
from conftest import load_pkg, make_scene

pytestmark = pytest.mark.gpu

TOL_DB = 1e-6
WORST = {}              # (what, route) -> largest |device - reference| in dB
NAMES = {0: "music", 1: "dbf", 2: "mvdr"}


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def _scan(pkg, ctx, method, n_dets, rp, ra):
    """One stand-alone DoA call; returns the device spectrum after checking the host tail against it."""
    doa = pkg.sensing.estimation.doaEstimation
    if method == 0:
        n_sig, azi, ele = doa.music(n_dets, rp, ra, ctx=ctx)
        assert n_sig == n_dets
    else:
        azi, ele = (doa.digitalBF if method == 1 else doa.mvdrBF)(n_dets, rp, ra, ctx=ctx)
    spec = ctx.angular_spectrum()
    _, locs = O.findpeaks(spec, npeaks=n_dets)
    assert np.array_equal(azi, locs * rp.azimuthScanGranularity - rp.azimuthScanScale / 2.0), (method, n_dets, azi)
    assert ele.size == azi.size and np.all(np.isnan(ele))
    return spec, azi


def _compare(spec, ref, what, route, tag):
    d = R.deviation(spec, ref)
    print(f"{what} route {route} {tag}: {d:.3e} dB")
    WORST[(what, route)] = max(WORST.get((what, route), 0.0), d)
    assert d <= TOL_DB, (what, route, tag, d)


def _record(record_property):
    for (what, route), d in sorted(WORST.items()):
        record_property(f"max_dev_db_{what}_route{route}", d)


@pytest.mark.parametrize("a", R.ARRAY_SIZES)
def test_prescribed_eigenstructure(pkg, a, record_property):
    ctx = pkg.Context()
    rp = R.rp_ula(n_ants=a)
    for spread in (R.SPREADS if a > 1 else R.SPREADS[:1]):
        c = R.prescribed_case(a, spread)
        for route in (0, 1):
            ctx.set_music_route(route)
            for n_sig in (R.music_num_dets(a, c.n_src) if spread == R.MUSIC_SPREAD or a == 1 else [max(c.n_src, 1)]):
                spec, azi = _scan(pkg, ctx, 0, n_sig, rp, c.ra)
                if n_sig >= a:                                            # empty noise space: flat 0 dB, no peaks
                    assert np.all(spec == 0.0) and azi.size == 0
                _compare(spec, R.prescribed_spectrum(c, 0, n_sig), "music", route, f"A={a} spread={spread:g} L={n_sig}")
        ctx.set_music_route(0)
        for method in (1, 2):
            spec, _ = _scan(pkg, ctx, method, max(c.n_src, 1), rp, c.ra)
            _compare(spec, R.prescribed_spectrum(c, method), NAMES[method], "-", f"A={a} spread={spread:g}")
    ctx.close()
    _record(record_property)


@pytest.mark.parametrize("name", sorted(R.PHYSICAL))
def test_physical_covariances(pkg, name, record_property):
    c = R.physical_case(name)
    ctx = pkg.Context()
    rp = R.rp_ula(n_ants=c.A)
    lists = {}
    for route in (0, 1):
        ctx.set_music_route(route)
        for n_sig in (1, c.n_src):
            spec, azi = _scan(pkg, ctx, 0, n_sig, rp, c.ra)
            _compare(spec, R.physical_spectrum(c, 0, n_sig), "music", route, f"{name} L={n_sig}")
        lists[(0, route)] = tuple(azi)
    for method in (1, 2):
        spec, azi = _scan(pkg, ctx, method, c.n_src, rp, c.ra)
        _compare(spec, R.physical_spectrum(c, method), NAMES[method], "-", name)
        lists[(method, 0)] = tuple(azi)
    if name == "close3":                                                    # the three methods disagree on the estimates, the device follows each
        want = [tuple(O.findpeaks(R.physical_spectrum(c, m, 2), npeaks=2)[1] - 180.0) for m in (0, 1, 2)]
        assert len(set(want)) == 3
        assert [lists[(0, 0)], lists[(1, 0)], lists[(2, 0)]] == want and lists[(0, 1)] == want[0]
    ctx.close()
    _record(record_property)


def test_non_default_scans_on_one_context(pkg, record_property):
    """362 steps of 0.5 degrees (none at +-90 ... the last one at 90.5) and 180 steps of 2 degrees after the default grid, then the default again."""
    c = R.prescribed_case(16, R.MUSIC_SPREAD)
    ctx = pkg.Context()
    for gran, scale, steps in ((1.0, 360.0, 361), (0.5, 180.0, 362), (2.0, 360.0, 180), (1.0, 360.0, 361), (0.5, 180.0, 362)):
        rp = R.rp_ula(gran, scale)
        for route in (0, 1):
            ctx.set_music_route(route)
            spec, _ = _scan(pkg, ctx, 0, c.n_src, rp, c.ra)
            assert spec.size == steps
            _compare(spec, R.prescribed_spectrum(c, 0, c.n_src, gran, scale), "music", route, f"grid {gran}/{scale}")
        for method in (1, 2):
            spec, _ = _scan(pkg, ctx, method, c.n_src, rp, c.ra)
            assert spec.size == steps
            _compare(spec, R.prescribed_spectrum(c, method, None, gran, scale), NAMES[method], "-", f"grid {gran}/{scale}")
    ctx.close()
    _record(record_property)


# ---------------------------------------------------------------------------------------------------------------- the chain
# Noisy scenes (the unit noise draw scaled up until the covariance has a noise FLOOR): the number of range estimates, which fft2D hands to MUSIC as L,
# then splits the eigenvalues at a gap >= 1e-3 w[0] -- at the default noise level the sidelobe detections put the split inside a floor 1e-9 w[0] wide.
CHAIN = {8: (dict(targets=((150.0, 40.0, 1.5), (-90.0, 70.0, 5.0)), velocity=(0.0, 6.0)), 3000.0),
         65: (dict(targets=((150.0, 40.0, 1.5),), velocity=(0.0,)), 1000.0)}


def _chain_scene(a):
    kw, noise_gain = CHAIN[a]
    sc = make_scene(n_ants=a, n_slots=2, nrb=24, num_slots_param=3, zero_s_slots=False, seed=21, **kw)
    echo = O.mono_static_sensing(sc.tx_wave, sc.tx_grid.shape, sc.carrier, sc.rp, sc.los, sc.noise * noise_gain, nfft=sc.wave.Nfft)
    return sc, echo


def _chain_reference(ra_dev, n_sig):
    a = ra_dev.shape[0]
    if a <= 16:
        w, v = R.mp_eigh_desc(ra_dev)
        return R.spectra_from_projections(w, R.projections(v, R.scan_angles()), 0, n_sig)
    return R.sign_projector_music(ra_dev, n_sig)


@pytest.mark.parametrize("a", sorted(CHAIN))
def test_fft2d_chain_spectrum(pkg, a, record_property):
    """fft2D's own scan (the fused pipeline, numDets on the device): dbg.spectrum_db against the reference spectrum of dbg.Ra at L = rngEst.size."""
    sc, echo = _chain_scene(a)
    w = np.linalg.eigvalsh(O.covariance(echo))[::-1]
    for route in (0, 1):
        ctx = pkg.Context()
        ctx.set_music_route(route)
        rp = pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)
        est, dbg = pkg.sensing.estimation.fft2D(rp, pkg.sensing.detection.cfar2D(rp), ctx.to_device(echo), ctx.to_device(sc.tx_grid), return_debug=True)
        n_sig = est.rngEst.size
        assert 0 < n_sig < a and w[n_sig - 1] - w[n_sig] >= 1e-3 * w[0], (n_sig, w[:8] / w[0])    # the gap condition, on the oracle's Ra
        assert np.array_equal(dbg.spectrum_db, ctx.angular_spectrum()) and dbg.spectrum_db.size == 361
        _compare(dbg.spectrum_db, _chain_reference(dbg.Ra, n_sig), "music_chain", route, f"A={a} L={n_sig}")
        _, locs = O.findpeaks(dbg.spectrum_db, npeaks=n_sig)
        assert np.array_equal(est.aziEst, locs - 180.0)
        ctx.close()
    _record(record_property)


# ---------------------------------------------------------------------------------------------------------------- the getter's contract
def _no_spectrum(pkg, ctx):
    with pytest.raises(pkg.IsacError) as ei:
        ctx.angular_spectrum()
    return ei.value.name == "INVALID_ARG"


def test_getter_contract(pkg):
    """isac_fft2d_get_music_spectrum hands out the context's LAST ULA azimuth scan, whichever call ran it, and nothing else."""
    est_pkg = pkg.sensing.estimation
    ctx = pkg.Context()
    assert _no_spectrum(pkg, ctx)                                           # a context with no ULA scan
    c16 = R.physical_case("a16")
    rp16 = R.rp_ula(n_ants=16)
    # a fresh context, then stand-alone digitalBF: the DBF spectrum (no fft2D has run)
    est_pkg.doaEstimation.digitalBF(2, rp16, c16.ra, ctx=ctx)
    assert R.deviation(ctx.angular_spectrum(), R.physical_spectrum(c16, 1)) <= TOL_DB
    assert R.deviation(ctx.angular_spectrum(), R.physical_spectrum(c16, 0, 2)) > 1.0
    # fft2D, then mvdrBF on another Ra: first fft2D's MUSIC spectrum, then the MVDR spectrum of that Ra
    sc, echo = _chain_scene(8)
    rp = pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)
    cf = pkg.sensing.detection.cfar2D(rp)
    d_echo, d_tx = ctx.to_device(echo), ctx.to_device(sc.tx_grid)
    est, dbg = est_pkg.fft2D(rp, cf, d_echo, d_tx, return_debug=True)
    assert R.deviation(ctx.angular_spectrum(), _chain_reference(dbg.Ra, est.rngEst.size)) <= TOL_DB
    est_pkg.doaEstimation.mvdrBF(2, rp16, c16.ra, ctx=ctx)
    assert R.deviation(ctx.angular_spectrum(), R.physical_spectrum(c16, 2)) <= TOL_DB
    # ... while the other getters still describe the fft2D
    dbg2 = import_module(pkg.__name__ + ".sensing.estimation.fft2D").fft2D_debug(ctx, 8)
    assert np.array_equal(dbg2.Ra, dbg.Ra) and np.array_equal(dbg2.power_window, dbg.power_window) and dbg2.spectrum_db.size == 361
    # then music2D: its AZIMUTH spectrum, n_steps long (not the range spectrum)
    rx = echo
    want, odbg = O.music2d(sc.rp, 30, rx, sc.tx_grid, return_debug=True)
    got = est_pkg.music2D(rp, SimpleNamespace(scs=30), rx, sc.tx_grid, ctx=ctx)
    spec = ctx.angular_spectrum()
    assert got.L == odbg.L and spec.size == 361
    _, locs = O.findpeaks(spec, npeaks=got.L)
    assert np.array_equal(got.aziEst, locs - 180.0)
    w = np.linalg.eigvalsh(odbg.Ra)[::-1]
    assert 0 < got.L < 8 and w[got.L - 1] - w[got.L] >= 1e-3 * w[0]
    assert R.deviation(spec, R.sign_projector_music(odbg.Ra, got.L)) <= TOL_DB
    # a refused UPA fft2D: the getter reports no spectrum
    rp_upa = copy.copy(rp)
    rp_upa.antennaType = SimpleNamespace(kind="upa", nV=2, nH=4)
    with pytest.raises(pkg.IsacError) as ei:
        est_pkg.fft2D(rp_upa, cf, d_echo, d_tx)
    assert ei.value.name == "UNSUPPORTED"
    assert _no_spectrum(pkg, ctx)
    # ... and a ULA scan after it is readable again
    est_pkg.doaEstimation.digitalBF(2, rp16, c16.ra, ctx=ctx)
    assert ctx.angular_spectrum().size == 361
    # isac_ctx_reserve's dry run is not a scan of the caller's: it leaves none behind
    pkg.sensing.reserve(sc.T, sc.tx_grid.shape, sc.carrier, rp, cf, nfft=sc.wave.Nfft, ctx=ctx)
    assert _no_spectrum(pkg, ctx)
    ctx.close()


def test_zz_report():
    print("\nULA DoA spectra, largest |device - reference| in dB: " + ", ".join(f"{w} route {r}: {d:.2e}" for (w, r), d in sorted(WORST.items())))
    assert WORST
