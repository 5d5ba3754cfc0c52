"""UPA direction finding on the GPU (ISAC_OPT_UPA_DOA, csrc/doa2d.hip) against the NumPy restatement of the reference's UPA branch
(tests/_upa_restatement.py: music.m:31-71, digitalBF.m:13-53, mvdrBF.m:13-53, the project's find2DPeaks):
  * isac_music_doa (both MUSIC routes, numDets given and []) and isac_beamscan_doa (DBF, MVDR) at 4 x 4, 8 x 8, 16 x 16 and 4 x 8: the dB map to <= 1e-6 dB,
    the estimates identical, mirror twins bitwise equal in the device map;
  * the whole chain at 8 x 8 (lazy monoStaticSensing -> fft2D) against the oracle's range-Doppler / CFAR / covariance stages, and through isac_sensing_submit_n;
  * tools.find2DPeaks on restated maps;
  * the option off: ISAC_ERR_UNSUPPORTED as before, and a ULA CPI unchanged by the option.
A scene whose peak order is decided by rounding (two ranked candidates, not twins, within 1e-6 dB of each other across the cut at L) is compared as a set within
tolerance and tallied, the way test_gpu_fuzz.py tallies "stage_at_rank"."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest

import _upa_restatement as R
from conftest import load_pkg, make_scene

pytestmark = pytest.mark.gpu

TOL_DB = 1e-6
TALLY = {"exact": 0, "rounding_defined": 0}


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def _rp(n_v, n_h):
    return SimpleNamespace(nIFFT=4096, nFFT=64, rRes=1.0, vRes=1.0, antennaType=SimpleNamespace(kind="upa", nV=n_v, nH=n_h),
                           azimuthScanScale=360, azimuthScanGranularity=1, elevationScanScale=180, elevationScanGranularity=1)


def _covariance(n_v, n_h, n_src, seed):
    """Sample covariance of n_src planted sources (off-grid directions) plus white noise, 4 A snapshots (full rank)."""
    rng = np.random.default_rng(seed)
    A = n_v * n_h
    N = 4 * A
    x = 0.1 * (rng.standard_normal((A, N)) + 1j * rng.standard_normal((A, N)))
    for _ in range(n_src):
        ph = R.steering_phases(n_v, n_h, np.array([rng.uniform(-70, 70)]), np.array([rng.uniform(-170, 170)]))[0]
        s = rng.uniform(0.5, 2.0) * (rng.standard_normal(N) + 1j * rng.standard_normal(N))
        x += np.exp(1j * ph)[:, None] * s[None, :]
    ra = x @ x.conj().T / N
    return np.asfortranarray(0.5 * (ra + ra.conj().T))


def _rounding_defined(pdb, n):
    """Does the order of the first n + 1 ranked candidates of pdb hinge on a difference <= TOL_DB between candidates that are not exact twins?"""
    ele, azi = R.find_2d_peaks(pdb, 10 ** 6)
    v = pdb[ele - 1, azi - 1][: n + 1]
    d = np.diff(v)
    return bool(np.any((d != 0) & (np.abs(d) <= TOL_DB)))


def _compare_estimates(dev_azi, dev_ele, ref_azi, ref_ele, ref_pdb, n):
    if np.array_equal(dev_azi, ref_azi) and np.array_equal(dev_ele, ref_ele):
        TALLY["exact"] += 1
        return
    assert _rounding_defined(ref_pdb, n), (dev_azi, dev_ele, ref_azi, ref_ele)
    TALLY["rounding_defined"] += 1
    got = np.sort(ref_pdb[(dev_ele + 90).astype(int), (dev_azi + 180).astype(int)])
    want = np.sort(ref_pdb[(ref_ele + 90).astype(int), (ref_azi + 180).astype(int)])
    assert got.size == want.size and np.abs(got - want).max() <= TOL_DB


def _check_map(ctx, ref_pdb):
    dev = ctx.angular_spectrum2d()
    assert dev.shape == ref_pdb.shape == (181, 361)
    assert np.abs(dev - ref_pdb).max() <= TOL_DB
    assert np.array_equal(dev, dev[::-1, R.twin_columns(361)])              # mirror twins bitwise equal
    assert np.all(dev.min(axis=0) == 0.0)                                   # column normalisation (music.m:61-63)
    return dev


SHAPES = [(4, 4), (8, 8), (16, 16), (4, 8)]
CASES = [("music", 0, True), ("music", 0, False), ("music", 1, True), ("music", 1, False), ("dbf", 0, True), ("mvdr", 0, True)]


@pytest.mark.parametrize("n_v,n_h", SHAPES)
@pytest.mark.parametrize("method,route,given", CASES)
def test_doa_against_restatement(pkg, n_v, n_h, method, route, given):
    ctx = pkg.Context()
    ctx.set_upa_doa(True)
    ctx.set_music_route(route)
    rp = _rp(n_v, n_h)
    for n_src in (1, 2, 3):
        ra = _covariance(n_v, n_h, n_src, seed=1000 * n_v + 10 * n_h + n_src)
        doa = pkg.sensing.estimation.doaEstimation
        if method == "music":
            nd = n_src if given else None
            L, azi, ele = doa.music(nd if given else [], rp, ra, ctx=ctx)
            L_ref, azi_ref, ele_ref, pdb = R.doa(0, ra, n_v, n_h, rp, num_dets=nd)
            assert L == L_ref
        else:
            m = 1 if method == "dbf" else 2
            azi, ele = (doa.digitalBF if m == 1 else doa.mvdrBF)(n_src, rp, ra, ctx=ctx)
            L_ref, azi_ref, ele_ref, pdb = R.doa(m, ra, n_v, n_h, rp, num_dets=n_src)
            L = n_src
        assert np.all(np.isfinite(ele)) and azi.size == ele.size
        _check_map(ctx, pdb)
        _compare_estimates(azi, ele, azi_ref, ele_ref, pdb, L)
    ctx.close()


def test_find2dpeaks_on_restated_maps(pkg):
    for seed, method in ((1, 0), (2, 1), (3, 2)):
        ra = _covariance(4, 4, 2, seed)
        pdb, _ = R.spectrum_db(method, ra, 4, 4, _rp(4, 4), num_dets=2)
        for n in (1, 4, 50):
            ele, azi = pkg.tools.find2DPeaks(pdb, n)
            e_ref, a_ref = R.find_2d_peaks(pdb, n)
            assert np.array_equal(ele, e_ref) and np.array_equal(azi, a_ref)
    m = np.zeros((5, 6))
    m[0, 2], m[2, 2], m[2, 4], m[1, 1] = 9.0, 3.0, 3.0, 1.0
    ele, azi = pkg.tools.find2DPeaks(m, 5)
    assert list(ele) == [3, 3] and list(azi) == [3, 5]
    with pytest.raises(pkg.IsacError) as ei:
        pkg.tools.find2DPeaks(m, 0)
    assert ei.value.name == "NO_DETECTION"


def test_option_off_is_unchanged(pkg):
    ctx = pkg.Context()
    rp = _rp(4, 4)
    ra = _covariance(4, 4, 1, 7)
    doa = pkg.sensing.estimation.doaEstimation
    for call in (lambda: doa.music(1, rp, ra, ctx=ctx), lambda: doa.digitalBF(1, rp, ra, ctx=ctx), lambda: doa.mvdrBF(1, rp, ra, ctx=ctx)):
        with pytest.raises(pkg.IsacError) as ei:
            call()
        assert ei.value.name == "UNSUPPORTED"
    # a ULA: bit-identical estimates with the option at 0 and at 1
    rp_ula = SimpleNamespace(nIFFT=4096, nFFT=64, rRes=1.0, vRes=1.0, antennaType=SimpleNamespace(kind="ula", numElements=16),
                             azimuthScanScale=360, azimuthScanGranularity=1, elevationScanScale=180, elevationScanGranularity=1)
    x = np.random.default_rng(8).standard_normal((16, 64)) + 1j * np.random.default_rng(9).standard_normal((16, 64))
    ra_ula = np.asfortranarray(x @ x.conj().T / 64)
    outs = []
    for on in (False, True):
        ctx.set_upa_doa(on)
        outs.append((doa.music(3, rp_ula, ra_ula, ctx=ctx), doa.digitalBF(3, rp_ula, ra_ula, ctx=ctx), doa.mvdrBF(3, rp_ula, ra_ula, ctx=ctx)))
    (m0, d0, v0), (m1, d1, v1) = outs
    assert m0[0] == m1[0] and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(m0[1:] + d0 + v0, m1[1:] + d1 + v1))
    ctx.close()


def _upa_scene(seed, targets=((120.0, 60.0, 1.5), (-250.0, 80.0, 1.5)), velocity=(10.0, -6.0)):
    sc = make_scene(n_ants=64, n_slots=4, nrb=273, targets=targets, velocity=velocity, seed=seed, zero_s_slots=False, with_noise=False)
    sc.cell.gNBSenAntenna = SimpleNamespace(kind="upa", nV=8, nH=8, dV=0.5, dH=0.5)
    return sc


def test_full_chain_8x8(pkg):
    """Lazy monoStaticSensing -> fft2D(reuse_range=True) on an 8 x 8 UPA: CFAR lists and range / velocity estimates equal the oracle's stages on the materialised
    grid, Ra to 1e-10, angles equal the restatement on that Ra; with the option off the same CPI raises UNSUPPORTED."""
    import oracle as O
    from oracle.fft2d import detect_per_antenna, unique_stable
    sc = _upa_scene(71)
    ctx = pkg.Context()
    rp = pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)
    rp_o = O.radar_params(sc.cell, sc.carrier, sc.wave)
    cf = pkg.sensing.detection.cfar2D(rp)
    d_wave, d_txg = ctx.to_device(sc.tx_wave), ctx.to_device(sc.tx_grid)
    run = lambda: pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, nfft=4096, fuse_fft2d=(rp, cf, d_txg), ctx=ctx, lazy=True, seed=9,
                                                noise_domain="spectral")
    lz = run()
    with pytest.raises(pkg.IsacError) as ei:
        pkg.sensing.estimation.fft2D(rp, cf, lz, d_txg, reuse_range=True)
    assert ei.value.name == "UNSUPPORTED"
    ctx.set_upa_doa(True)
    lz = run()
    est, dbg = pkg.sensing.estimation.fft2D(rp, cf, lz, d_txg, reuse_range=True, return_debug=True)
    grid = lz.materialize().numpy()
    rdm = O.rdm_explicit(grid, sc.tx_grid, int(rp_o.nIFFT), int(rp_o.nFFT))
    dets, all_rng, all_vel = detect_per_antenna(rdm, O.cfar2d_config(rp_o), rp_o.rRes, rp_o.vRes, int(rp_o.nFFT))
    assert all(np.array_equal(a, b) for a, b in zip(dbg.detections, dets))
    rng_ref, vel_ref = unique_stable(all_rng), unique_stable(all_vel)
    assert np.array_equal(est.rngEst, rng_ref) and np.array_equal(est.velEst, vel_ref)
    ra_ref = O.covariance(grid)
    assert np.abs(dbg.Ra - ra_ref).max() <= 1e-10 * np.abs(ra_ref).max()
    assert rng_ref.size > 0
    _, azi_ref, ele_ref, pdb = R.doa(0, dbg.Ra, 8, 8, rp, num_dets=rng_ref.size)
    assert np.abs(dbg.spectrum_db_2d - pdb).max() <= TOL_DB
    assert np.array_equal(dbg.spectrum_db_2d, dbg.spectrum_db_2d[::-1, R.twin_columns(361)])
    _compare_estimates(est.aziEst, est.eleEst, azi_ref, ele_ref, pdb, rng_ref.size)
    ctx.close()


def test_submit_n_matches_single_calls(pkg):
    scs = [_upa_scene(80 + i, targets=((120.0 + 15 * i, 60.0, 1.5), (-250.0, 80.0 - 5 * i, 1.5))) for i in range(4)]
    ctxs = [pkg.Context() for _ in scs]
    for c in ctxs:
        c.set_upa_doa(True)
    rps = [pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave) for sc in scs]
    cf = pkg.sensing.detection.cfar2D(rps[0])
    waves = [c.to_device(sc.tx_wave) for c, sc in zip(ctxs, scs)]
    grids = [c.to_device(sc.tx_grid) for c, sc in zip(ctxs, scs)]
    los = [np.ones(2, np.uint8)] * 4
    res = pkg.sensing.submitN(ctxs, waves, grids, scs[0].tx_grid.shape, scs[0].carrier, rps, los, cf, seeds=[21, 22, 23, 24], nfft=4096).collect()
    n_ok = 0
    for i in range(4):
        lz = pkg.sensing.monoStaticSensing(waves[i], scs[i].tx_grid.shape, scs[i].carrier, rps[i], los[i], nfft=4096, fuse_fft2d=(rps[i], cf, grids[i]), ctx=ctxs[i],
                                           lazy=True, seed=21 + i, noise_domain="spectral")
        try:
            want = pkg.sensing.estimation.fft2D(rps[i], cf, lz, grids[i], reuse_range=True)
        except pkg.IsacError as e:
            assert isinstance(res[i], pkg.IsacError) and res[i].name == e.name
            continue
        got = res[i]
        assert not isinstance(got, Exception), got
        assert all(np.array_equal(getattr(got, k), getattr(want, k)) for k in ("rngEst", "velEst", "aziEst", "eleEst"))
        assert np.all(np.isfinite(got.eleEst))
        n_ok += 1
    assert n_ok >= 2
    for c in ctxs:
        c.close()


def test_zz_tally():
    total = TALLY["exact"] + TALLY["rounding_defined"]
    print(f"\nUPA DoA tally: exact {TALLY['exact']}, rounding-defined {TALLY['rounding_defined']} of {total} scenes")
    assert total > 0 and TALLY["rounding_defined"] <= max(2, total // 10)
