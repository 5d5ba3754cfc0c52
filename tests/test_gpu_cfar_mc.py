"""isac_cfar_monte_carlo on the MI355X (include/isac_cfar_mc.h; project-defined): the per-trial flags against the NumPy restatement
(tests/_cfar_mc_restatement.py), independence of the launch geometry, and the counted false-alarm and detection rates of the library's own detectors with their 'Auto'
factors against the expressions written out in the restatement -- |d - n p| <= 5 sqrt(n p (1 - p)) throughout, seeds fixed."""
from __future__ import annotations

import ctypes as C
import math
import time
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest

import _cfar_mc_restatement as MC
import _target_list_restatement as R

pytestmark = pytest.mark.gpu

CODE = {"CA": 0, "GOCA": 1, "SOCA": 2, "OS": 3}
INVALID_ARG, UNSUPPORTED = 1, 7
N_FLAG_TRIALS = 1 << 16
FLAG_SNR = [-np.inf, 0.0, 10.0, 13.0]
FLAG_CASES = [("CA", 2, 1), ("CA", 24, 1), ("GOCA", 24, 1), ("SOCA", 24, 1), ("OS", 24, 18), ("OS", 24, 1), ("OS", 24, 24), ("CA", 56, 1), ("OS", 56, 42), ("CA", 128, 1)]
SEED = 20240611


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context()
    yield c
    c.close()


def _mc(pkg, ctx, method, N, rank, custom, pfa, model, snr, n_trials, seed, want_flags=False, n_snr=None):
    """isac_cfar_monte_carlo through ctypes: (status, n_det [n_snr] uint64, flags [n_trials x n_snr] or None)."""
    L = pkg._lib
    m = L.CfarMethod(CODE[method] if isinstance(method, str) else method, rank, custom)
    s = np.ascontiguousarray(snr, dtype=np.float64)
    n_snr = s.size if n_snr is None else n_snr
    n_det = np.full(max(n_snr, s.size, 1), 2 ** 64 - 1, dtype=np.uint64)
    flags = np.full((n_trials, max(n_snr, 1)), 7, dtype=np.uint8, order="F") if want_flags else None
    st = ctx.lib.isac_cfar_monte_carlo(ctx.handle, C.byref(m), N, pfa, MC.MODELS[model] if isinstance(model, str) else model, s.ctypes.data_as(C.c_void_p), n_snr, n_trials,
                                       seed, n_det.ctypes.data_as(C.c_void_p), None if flags is None else flags.ctypes.data_as(C.c_void_p))
    return st, n_det[:max(n_snr, 0)], flags


def _alpha(pkg, method, N, pfa, rank):
    return pkg.sensing.detection.cfarThresholdFactor(method, N, pfa, Rank=rank)


def _check_flags(pkg, ctx, method, N, rank, custom, pfa, model, n_trials=N_FLAG_TRIALS):
    alpha = custom if custom else _alpha(pkg, method, N, pfa, rank)
    want, margin = MC.detect(MC.cached_draw(N, SEED, n_trials), method, rank, alpha, model, FLAG_SNR)
    keep = margin > MC.MARGIN
    assert (~keep).sum() <= 2, (method, N, rank, model, int((~keep).sum()))   # the restatement alone; zero is expected
    st, n_det, flags = _mc(pkg, ctx, method, N, rank, custom, pfa, model, FLAG_SNR, n_trials, SEED, want_flags=True)
    assert st == 0 and set(np.unique(flags)) <= {0, 1}
    assert np.array_equal(flags[keep], want[keep]), (method, N, rank, custom, model, int((flags != want).sum()))
    assert np.array_equal(n_det, flags.sum(axis=0, dtype=np.uint64))
    return flags, n_det


@pytest.mark.parametrize("method,N,rank", FLAG_CASES)
def test_flags_equal_the_restatement(pkg, ctx, method, N, rank):
    seen = 0
    for model in MC.MODELS:
        for custom, pfa in ((0.0, 1e-2), (5.0, 0.5)):
            flags, n_det = _check_flags(pkg, ctx, method, N, rank, custom, pfa, model)
            print(f"{method} N {N} rank {rank} {model} {'Auto' if not custom else 'Custom 5.0'}: n_det {n_det.tolist()}")
            assert (np.diff(n_det.astype(np.int64)) >= 0).all()                # common random numbers: non-decreasing in SNR
            seen += int(n_det.sum())
    assert seen > 0


@pytest.mark.parametrize("method,N,rank", [("CA", 24, 1), ("OS", 24, 18), ("SOCA", 56, 1), ("CA", 128, 1)])
def test_geometry_independence(pkg, ctx, method, N, rank):
    """A run that ends in the middle of a workgroup, a run shorter than one workgroup's pass and a counts-only call: the same trials give the same flags."""
    base, base_det = _check_flags(pkg, ctx, method, N, rank, 0.0, 1e-2, "swerling0")
    st, det_l, longer = _mc(pkg, ctx, method, N, rank, 0.0, 1e-2, "swerling0", FLAG_SNR, N_FLAG_TRIALS + 37, SEED, want_flags=True)
    assert st == 0 and np.array_equal(longer[:N_FLAG_TRIALS], base) and np.array_equal(det_l, longer.sum(axis=0, dtype=np.uint64))
    st, det_s, short = _mc(pkg, ctx, method, N, rank, 0.0, 1e-2, "swerling0", FLAG_SNR, 1000, SEED, want_flags=True)
    assert st == 0 and np.array_equal(short, base[:1000]) and np.array_equal(det_s, short.sum(axis=0, dtype=np.uint64))
    for n, want in ((N_FLAG_TRIALS, base_det), (N_FLAG_TRIALS + 37, det_l), (1000, det_s), (1, base[:1].sum(axis=0, dtype=np.uint64))):
        st, det, none = _mc(pkg, ctx, method, N, rank, 0.0, 1e-2, "swerling0", FLAG_SNR, n, SEED)
        assert st == 0 and none is None and np.array_equal(det, want), n
    st, det, _ = _mc(pkg, ctx, method, N, rank, 0.0, 1e-2, "swerling0", FLAG_SNR, N_FLAG_TRIALS, SEED + 1)
    assert st == 0 and not np.array_equal(det, base_det)                      # the seed matters


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("method", ["CA", "GOCA", "SOCA", "OS"])
def test_false_alarm_rate_of_the_auto_factor(pkg, ctx, method, seed):
    """N = 24 (OS rank 18), snr_db = [-inf]: Pfa 1e-3 over 2^26 trials and Pfa 1e-5 over 2^30 trials (four launches) within 5 sigma."""
    for pfa, n in ((1e-3, 1 << 26), (1e-5, 1 << 30)):
        t = time.perf_counter()
        st, det, _ = _mc(pkg, ctx, method, 24, 18, 0.0, pfa, "swerling0", [-np.inf], n, seed)
        dt = time.perf_counter() - t
        assert st == 0
        ok, z = MC.within_5_sigma(int(det[0]), n, pfa)
        print(f"{method} seed {seed} Pfa {pfa:g}: {int(det[0])} of 2^{n.bit_length() - 1}, {z:+.2f} sigma, {dt:.3f} s")
        assert ok, (method, seed, pfa, int(det[0]), z)


@pytest.mark.parametrize("method", ["CA", "GOCA", "SOCA", "OS"])
def test_pd_swerling1(pkg, ctx, method):
    N, rank, pfa, n, snr = 24, 18, 1e-4, 1 << 24, [0.0, 5.0, 10.0, 15.0, 20.0]
    want = MC.pd_swerling1(method, N, _alpha(pkg, method, N, pfa, rank), rank, snr)
    st, det, _ = _mc(pkg, ctx, method, N, rank, 0.0, pfa, "swerling1", snr, n, 1)
    assert st == 0 and (np.diff(det.astype(np.int64)) >= 0).all()
    for x, d, p in zip(snr, det, want):
        ok, z = MC.within_5_sigma(int(d), n, float(p))
        print(f"{method} Swerling 1 {x} dB: Pd {int(d) / n:.6f}, expression {p:.6f}, {z:+.2f} sigma")
        assert ok, (method, x, int(d), p)


def test_pd_swerling0_ca(pkg, ctx):
    N, pfa, n, snr = 24, 1e-3, 1 << 24, [0.0, 5.0, 10.0, 13.0]
    want = MC.pd_swerling0_ca(N, _alpha(pkg, "CA", N, pfa, 1), snr)
    st, det, _ = _mc(pkg, ctx, "CA", N, 1, 0.0, pfa, "swerling0", snr, n, 1)
    assert st == 0 and (np.diff(det.astype(np.int64)) >= 0).all()
    for x, d, p in zip(snr, det, want):
        ok, z = MC.within_5_sigma(int(d), n, float(p))
        print(f"CA Swerling 0 {x} dB: Pd {int(d) / n:.6f}, quadrature {p:.6f}, {z:+.2f} sigma")
        assert ok, (x, int(d), p)


def test_errors_leave_the_context_usable(pkg, ctx):
    nan, inf = math.nan, math.inf
    ok = dict(method="CA", N=24, rank=1, custom=0.0, pfa=1e-2, model="swerling0", snr=[0.0], n_trials=1000, seed=1)
    bad = [(dict(N=23), INVALID_ARG), (dict(N=1), INVALID_ARG), (dict(N=0), INVALID_ARG), (dict(N=130), UNSUPPORTED),
           (dict(method="OS", rank=0), INVALID_ARG), (dict(method="OS", rank=25), INVALID_ARG), (dict(method="GOCA", custom=-1.0), INVALID_ARG),
           (dict(method=4), INVALID_ARG), (dict(pfa=0.0), INVALID_ARG), (dict(snr=[0.0, nan]), INVALID_ARG), (dict(snr=[inf]), INVALID_ARG),
           (dict(snr=[0.0], n_snr=0), INVALID_ARG), (dict(snr=[0.0] * 65), INVALID_ARG), (dict(n_trials=(1 << 22) + 1, want_flags=True), INVALID_ARG),
           (dict(n_trials=0), INVALID_ARG), (dict(n_trials=(1 << 40) + 1), INVALID_ARG), (dict(model=2), INVALID_ARG)]
    for change, want in bad:
        st, det, _ = _mc(pkg, ctx, **{**ok, **change})
        assert st == want, (change, st)
        assert (det == np.uint64(2 ** 64 - 1)).all()                           # nothing written
        _check_flags(pkg, ctx, *FLAG_CASES[0], 0.0, 1e-2, "swerling0", n_trials=4096)
    assert ctx.lib.isac_cfar_monte_carlo(ctx.handle, None, 24, 1e-2, 0, None, 1, 1, 0, None, None) == INVALID_ARG
    st, det, flags = _mc(pkg, ctx, "OS", 128, 96, 0.0, 1e-2, "swerling1", [0.0] * 64, 1 << 10, 5, want_flags=True)   # the largest window, every SNR slot
    assert st == 0 and (det == det[0]).all() and np.array_equal(det, flags.sum(axis=0, dtype=np.uint64))
    # the Python entry: a cfarConfig gives N = 24 and its Pfa
    det2d = pkg.sensing.detection
    cf = SimpleNamespace(cfarDetector2D=det2d.CFARDetector2D(1e-2, (2, 2), (1, 1)))
    r = det2d.cfarMonteCarlo(cf, FLAG_SNR, N_FLAG_TRIALS, Method="OS", Rank=18, seed=SEED, return_flags=True, ctx=ctx)
    want, _ = MC.detect(MC.cached_draw(24, SEED, N_FLAG_TRIALS), "OS", 18, _alpha(pkg, "OS", 24, 1e-2, 18), "swerling0", FLAG_SNR)
    assert np.array_equal(r.nDet, want.sum(axis=0, dtype=np.uint64)) and r.alpha == _alpha(pkg, "OS", 24, 1e-2, 18) and r.nTrials == N_FLAG_TRIALS
    assert np.array_equal(r.Pd, r.nDet / N_FLAG_TRIALS) and np.allclose(r.stderr, np.sqrt(r.Pd * (1 - r.Pd) / N_FLAG_TRIALS)) and r.flags.shape == (N_FLAG_TRIALS, 4)
    c = det2d.cfarMonteCarlo(24, [0.0], 1000, ThresholdFactor="Custom", CustomThresholdFactor=5.0, model="swerling1", ctx=ctx)
    assert c.alpha == 5.0 and not hasattr(c, "flags")
    with pytest.raises(pkg.IsacError):
        det2d.cfarMonteCarlo(23, [0.0], 1000, Pfa=1e-2, ctx=ctx)
    with pytest.raises(ValueError):
        det2d.cfarMonteCarlo(24, [0.0], 1000, ctx=ctx)                         # 'Auto' without Pfa


def test_no_side_effect_on_the_last_fft2d(pkg):
    """redetect and targetList of a completed fft2D answer the same before and after Monte-Carlo calls on its context."""
    sc = R.make("a4_24prb_generic")
    rp = pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)
    cf = pkg.sensing.detection.cfar2D(rp)
    F = import_module(pkg.__name__ + ".sensing.estimation.fft2D")
    c = pkg.Context()
    try:
        d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
        echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c)
        est = pkg.sensing.estimation.fft2D(rp, cf, echo, d_txg, ctx=c)

        def state():
            e, dbg = pkg.sensing.estimation.redetect(c, Method="OS", Rank=18, return_debug=True)
            tl = pkg.sensing.estimation.targetList(c, snapshots=True)
            whole = F.fft2D_debug(c, sc.A)
            return ([e.rngEst, e.velEst, e.aziEst, np.concatenate(dbg.detections, axis=1), np.concatenate(dbg.det_pow), dbg.Ra, whole.power_window, whole.spectrum_db]
                    + [np.asarray(tl[k]) for k in sorted(tl)])
        before = state()
        assert before[3].shape[1] > 0 and before[-1].size > 0
        for method, N, rank, n, flags in (("CA", 24, 1, 1 << 20, False), ("OS", 24, 18, 1 << 16, True), ("GOCA", 128, 1, 1 << 12, True)):
            st, det, _ = _mc(pkg, c, method, N, rank, 0.0, 1e-2, "swerling1", FLAG_SNR, n, 3, want_flags=flags)
            assert st == 0 and det[-1] > 0
        after = state()
        assert len(before) == len(after) and all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
        # a pending submit and its result survive a call in between
        F.fft2D_submit(rp, cf, echo, d_txg, ctx=c)
        assert _mc(pkg, c, "SOCA", 24, 1, 0.0, 1e-2, "swerling0", FLAG_SNR, 1 << 16, 3, want_flags=True)[0] == 0
        est1 = F.fft2D_collect(c)
        for k in ("rngEst", "velEst", "aziEst"):
            assert getattr(est1, k).tobytes() == getattr(est, k).tobytes(), k
    finally:
        c.close()
