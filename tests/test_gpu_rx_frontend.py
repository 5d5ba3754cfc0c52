"""The tail of applyChannelModel on the device (csrc/rxfe.hip: isac_rx_frontend[_batch]_dev) and the Python / MEX layers above it, against the NumPy restatement
(tests/_rx_frontend_restatement.py), the oracle's Philox generator and the oracle's CDL apply.  Tolerance: RTOL = 1e-10 relative to the field's largest magnitude, the
project's bound for complex fp64 fields (README "Parity"); the kernel is two multiplies and one fused multiply-add per component, so ~1e-16 is expected."""
from __future__ import annotations

import ctypes as C
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import _rx_frontend_restatement as R
from conftest import ROOT, load_pkg
from oracle.philox import philox_normal_pairs

pytestmark = pytest.mark.gpu
RTOL = 1e-10
STREAM = 3                                  # kRxFrontEndStream (csrc/isac_internal.hpp)
PL_DB, GAIN_DB, FS = 120.0, 6.0, 122.88e6   # a scale pair far from 1; thermal noise at config 5's sample rate
NT = R.thermal_noise_power(290.0, 7.0, FS)
NONE, INJECTED, PHILOX, PHILOX_SPECTRAL, INJECTED_SPECTRAL = 0, 1, 2, 3, 4


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def ctx(pkg):
    return pkg.default_context()


def cplx(rng, shape):
    return np.asfortranarray(rng.standard_normal(shape) + 1j * rng.standard_normal(shape))


def front_end(ctx, d_y, s1, s2, nt, mode, d_w=None, seed=0):
    T, nr = d_y.shape
    return ctx.lib.isac_rx_frontend_dev(ctx.handle, C.c_void_p(d_y.ptr), C.c_int64(T), C.c_int32(nr), C.c_double(s1), C.c_double(s2), C.c_double(nt), C.c_int32(mode),
                                        C.c_void_p(d_w.ptr if d_w is not None else None), C.c_uint64(seed))


S1, S2 = 10.0 ** (-PL_DB / 20.0), 10.0 ** (GAIN_DB / 20.0)
SHAPES = [(6001, 2), (6001, 64), (61909, 2), (4097, 1)]


@pytest.mark.parametrize("T,nr", SHAPES)
def test_injected_noise_matches_the_restatement(ctx, T, nr):
    rng = np.random.default_rng(T + nr)
    x, w = cplx(rng, (T, nr)), cplx(rng, (T, nr))
    d_y, d_w = ctx.to_device(x), ctx.to_device(w)
    ctx.check(front_end(ctx, d_y, S1, S2, NT, INJECTED, d_w))
    want = R.rx_frontend(x, PL_DB, GAIN_DB, NT, w)
    err = rel(d_y.numpy(), want)
    print(f"injected [{T} x {nr}]: rel err {err:.3e}")
    assert err < RTOL
    assert np.array_equal(d_w.numpy(), w)                          # the noise buffer is read only


@pytest.mark.parametrize("T,nr", SHAPES)
def test_noiseless_scaling_and_identity(ctx, T, nr):
    rng = np.random.default_rng(7 * T + nr)
    x = cplx(rng, (T, nr))
    d_y = ctx.to_device(x)
    ctx.check(front_end(ctx, d_y, S1, S2, NT, NONE))
    err = rel(d_y.numpy(), (x * S1) * S2)
    print(f"noiseless [{T} x {nr}]: rel err {err:.3e}")
    assert err < RTOL
    d_z = ctx.to_device(x)
    ctx.check(front_end(ctx, d_z, 1.0, 1.0, NT, NONE))
    assert d_z.numpy().tobytes() == x.tobytes()                    # both scales 1: bit for bit


@pytest.mark.parametrize("T,nr", SHAPES)
def test_philox_noise_matches_the_restated_generator(ctx, T, nr):
    rng = np.random.default_rng(11 * T + nr)
    x = cplx(rng, (T, nr))
    seed = 0x1234_5678_9ABC_DEF0 + T
    d_y = ctx.to_device(x)
    ctx.check(front_end(ctx, d_y, S1, S2, NT, PHILOX, seed=seed))
    w = philox_normal_pairs(np.arange(T * nr, dtype=np.uint64), seed, STREAM).reshape((T, nr), order="F")      # element index e = t + T u
    got = d_y.numpy()
    err = rel(got, R.rx_frontend(x, PL_DB, GAIN_DB, NT, w))
    print(f"philox [{T} x {nr}]: rel err {err:.3e}")
    assert err < RTOL
    d_2 = ctx.to_device(x)
    ctx.check(front_end(ctx, d_2, S1, S2, NT, PHILOX, seed=seed))
    assert d_2.numpy().tobytes() == got.tobytes()                  # one seed: bit-identical
    d_3 = ctx.to_device(x)
    ctx.check(front_end(ctx, d_3, S1, S2, NT, PHILOX, seed=seed + 1))
    assert np.count_nonzero(d_3.numpy() != got) > 0.99 * got.size  # another seed: another field


def test_philox_unit_noise_statistics(ctx):
    """The unit noise recovered from a zero input on 6 001 x 64 = 384 064 samples: |std - 1| < 0.02 per component (the bound of tests/test_gpu_parity.py; one standard
    error at that count is 0.0011) -- asserted on the restated generator too, so the reference alone is shown to stay inside the bound."""
    T, nr, seed = 6001, 64, 20260101
    d_y = ctx.to_device(np.zeros((T, nr), dtype=np.complex128, order="F"))
    ctx.check(front_end(ctx, d_y, S1, S2, NT, PHILOX, seed=seed))
    unit = d_y.numpy() / math.sqrt(NT / 2.0)
    ref = philox_normal_pairs(np.arange(T * nr, dtype=np.uint64), seed, STREAM)
    for name, z in (("device", unit), ("restated generator", ref)):
        sr, si = float(np.std(z.real)), float(np.std(z.imag))
        print(f"{name}: std(re) {sr:.5f} std(im) {si:.5f} mean {abs(np.mean(z)):.2e}")
        assert abs(sr - 1.0) < 0.02 and abs(si - 1.0) < 0.02, (name, sr, si)
    assert rel(unit.ravel(order="F"), ref) < RTOL


def _views(ctx, pkg, T, nr, n, guard, fill):
    """n arrays [T x nr] inside ONE device allocation, `guard` elements in front of, between and behind them (filled with `fill`)."""
    per = T * nr
    host = np.full(guard + n * (per + guard), fill, dtype=np.complex128)
    offs = [guard + j * (per + guard) for j in range(n)]
    d_all = ctx.to_device(host)
    views = [pkg._lib.DeviceArray(ctx, d_all.ptr + 16 * o, (T, nr), np.complex128, owner=False) for o in offs]
    return d_all, host, offs, views


@pytest.mark.parametrize("mode", [NONE, INJECTED, PHILOX])
def test_batch_equals_single_calls_and_touches_nothing_else(pkg, ctx, mode):
    T, nr, n, guard = 4097, 3, 7, 37                               # odd T, odd guard: no job starts on more than the 16 B of an element
    rng = np.random.default_rng(100 + mode)
    fill = complex(float.fromhex("0x1.deadbeefp+3"), -float.fromhex("0x1.cafef00dp-2"))
    xs = [cplx(rng, (T, nr)) for _ in range(n)]
    ws = [cplx(rng, (T, nr)) for _ in range(n)]
    s1 = [10.0 ** (-(60.0 + 9.0 * j) / 20.0) for j in range(n)]
    s2 = [10.0 ** ((j - 3.0) / 20.0) for j in range(n)]
    nts = [R.thermal_noise_power(250.0 + 10.0 * j, 1.0 + j, FS / (1 + j % 3)) for j in range(n)]
    seeds = [1000 + 17 * j for j in range(n)]
    d_ws = [ctx.to_device(w) for w in ws] if mode == INJECTED else None
    # the seven single calls
    singles = []
    for j in range(n):
        d = ctx.to_device(xs[j])
        ctx.check(front_end(ctx, d, s1[j], s2[j], nts[j], mode, d_ws[j] if d_ws else None, seeds[j]))
        singles.append(d.numpy())
    # one batch, the arrays inside one allocation with guard rows around each
    d_all, host, offs, views = _views(ctx, pkg, T, nr, n, guard, fill)
    for v, x in zip(views, xs):
        ctx.check(ctx.lib.isac_memcpy_h2d(ctx.handle, C.c_void_p(v.ptr), x.ctypes.data_as(C.c_void_p), C.c_size_t(x.nbytes)))
        host[(v.ptr - d_all.ptr) // 16:(v.ptr - d_all.ptr) // 16 + T * nr] = x.ravel(order="F")
    jobs = (pkg._lib.RxFrontendJob * n)()
    for j in range(n):
        jobs[j] = pkg._lib.RxFrontendJob(views[j].ptr, d_ws[j].ptr if d_ws else None, s1[j], s2[j], nts[j], seeds[j])
    ctx.check(ctx.lib.isac_rx_frontend_batch_dev(ctx.handle, jobs, C.c_int32(n), C.c_int64(T), C.c_int32(nr), C.c_int32(mode)))
    after = d_all.numpy()
    inside = np.zeros(after.size, dtype=bool)
    for j, o in enumerate(offs):
        inside[o:o + T * nr] = True
        assert after[o:o + T * nr].tobytes() == singles[j].ravel(order="F").tobytes(), f"job {j} differs from its single call"
    assert after[~inside].tobytes() == host[~inside].tobytes(), "bytes outside the jobs' arrays were written"
    if mode != NONE:
        assert not np.array_equal(singles[0], (xs[0] * s1[0]) * s2[0])


GNB64, UE2 = (4, 8, 2, 1, 1), (1, 1, 2, 1, 1)
LINK = dict(path_loss_config="UMa", carrier_freq=3.5e9, rx_gain_db=GAIN_DB, noise_figure_db=7.0, temperature_k=290.0, sample_rate=15.36e6)
GNB_POS, UE_POS = (0.0, 0.0, 25.0), (120.0, 50.0, 1.5)


def _tail(y, los, own, other, w, cfg="UMa"):
    pl = R.fspl(3.5e9, own, other) if cfg == "fspl" else R.path_loss_38901(cfg, 3.5e9, los, own, other)
    return R.rx_frontend(y, pl, GAIN_DB, R.thermal_noise_power(290.0, 7.0, 15.36e6), w)


@pytest.mark.parametrize("profile,tx,rx,los", [("CDL-A", GNB64, UE2, 0), ("CDL-D", GNB64, UE2, 1), ("CDL-A", UE2, GNB64, 0), ("CDL-D", UE2, GNB64, 1)])
def test_apply_channel_model_with_a_cdl_channel(pkg, ctx, profile, tx, rx, los):
    import oracle.cdl as OC
    CM, PHY = pkg.communication.channelModels, pkg.communication.phyLayer
    fs, T = 15.36e6, 4097
    nt, nr = int(np.prod(tx)), int(np.prod(rx))
    down = nt > nr
    own, other = (UE_POS, GNB_POS) if down else (GNB_POS, UE_POS)         # the receiver's own node first: uePhy.m:744 / gNBPhy.m:853
    rng = np.random.default_rng(nt + 3 * nr + los)
    x, w = cplx(rng, (T, nt)), cplx(rng, (T, nr))
    cfg = OC.cdl_config(profile, 3.5e9, tx, rx, fs)
    want = _tail(OC.apply_cdl(cfg, x, 0.0), los, own, other, w)
    ch = CM.CDLChannel(profile, 300e-9, 3.5e9, tx, rx, fs)
    got = PHY.applyChannelModel(x, channel=ch, los=los, own_position=own, tx_position=other, noise=w, ctx=ctx, **LINK)            # host in, host out
    assert isinstance(got, np.ndarray) and got.shape == (T, nr)
    err = rel(got, want)
    print(f"applyChannelModel {profile} {nt} -> {nr}: rel err {err:.3e}")
    assert err < RTOL and ch.time == pytest.approx(T / fs)
    ch2 = CM.CDLChannel(profile, 300e-9, 3.5e9, tx, rx, fs)
    d_got = PHY.applyChannelModel(ctx.to_device(x), channel=ch2, los=los, own_position=own, tx_position=other, noise=ctx.to_device(w), ctx=ctx, **LINK)
    assert isinstance(d_got, pkg.DeviceArray) and np.array_equal(d_got.numpy(), got)                                               # device in, device out: the same values
    # the quirk of the downlink call is observable: the positions the other way round give another path loss (h_BS / h_UT swapped)
    if not los:
        ch3 = CM.CDLChannel(profile, 300e-9, 3.5e9, tx, rx, fs)
        sw = PHY.applyChannelModel(x, channel=ch3, los=los, own_position=other, tx_position=own, ctx=ctx, **LINK)
        assert rel(sw, _tail(OC.apply_cdl(cfg, x, 0.0), los, other, own, None)) < RTOL
        assert rel(sw, _tail(OC.apply_cdl(cfg, x, 0.0), los, own, other, None)) > 1e-3


@pytest.mark.parametrize("nt,nr,cfg", [(64, 2, "UMa"), (2, 64, "fspl"), (4, 4, "InH"), (1, 1, "RMa")])
def test_apply_channel_model_without_a_channel_object(pkg, ctx, nt, nr, cfg):
    PHY = pkg.communication.phyLayer
    T = 4097
    rng = np.random.default_rng(nt * 100 + nr)
    x, w = cplx(rng, (T, nt)), cplx(rng, (T, nr))
    link = dict(LINK, path_loss_config=cfg)
    want = _tail(x @ R.dft_channel_matrix(nt, nr), 1, UE_POS, GNB_POS, w, cfg)
    got = PHY.applyChannelModel(x, channel=None, n_rx=nr, los=1, own_position=UE_POS, tx_position=GNB_POS, noise=w, ctx=ctx, **link)
    err = rel(got, want)
    print(f"applyChannelModel DFT branch {nt} -> {nr} ({cfg}): rel err {err:.3e}")
    assert got.shape == (T, nr) and err < RTOL
    d_got = PHY.applyChannelModel(ctx.to_device(x), channel=None, n_rx=nr, los=1, own_position=UE_POS, tx_position=GNB_POS, noise=w, ctx=ctx, **link)
    assert np.array_equal(d_got.numpy(), got)
    seeded = PHY.applyChannelModel(x, channel=None, n_rx=nr, los=1, own_position=UE_POS, tx_position=GNB_POS, seed=5, ctx=ctx, **link)
    wp = philox_normal_pairs(np.arange(T * nr, dtype=np.uint64), 5, STREAM).reshape((T, nr), order="F")
    assert rel(seeded, _tail(x @ R.dft_channel_matrix(nt, nr), 1, UE_POS, GNB_POS, wp, cfg)) < RTOL


def test_apply_channel_model_batch_equals_the_single_calls(pkg, ctx):
    CM, PHY = pkg.communication.channelModels, pkg.communication.phyLayer
    fs, T, n = 15.36e6, 3001, 3
    rng = np.random.default_rng(5)
    x = cplx(rng, (T, 64))
    ws = [cplx(rng, (T, 2)) for _ in range(n)]
    ues = [(100.0 + 40.0 * j, -30.0 * j, 1.5) for j in range(n)]
    los = [0, 1, 0]
    d_x = ctx.to_device(x)
    mk = lambda: [CM.CDLChannel("CDL-A", 300e-9, 3.5e9, GNB64, UE2, fs, Seed=73 + j) for j in range(n)]
    outs = PHY.applyChannelModelBatch([d_x] * n, channels=mk(), los=los, own_positions=ues, tx_positions=[GNB_POS] * n, noises=[ctx.to_device(w) for w in ws], ctx=ctx, **LINK)
    for j, ch in enumerate(mk()):
        one = PHY.applyChannelModel(d_x, channel=ch, los=los[j], own_position=ues[j], tx_position=GNB_POS, noise=ws[j], ctx=ctx, **LINK)
        assert rel(outs[j].numpy(), one.numpy()) < RTOL            # (the batched and the single CDL apply may take different kernels: equal to rounding)


def test_errors_leave_the_context_usable(pkg, ctx):
    T, nr = 1000, 2
    x = cplx(np.random.default_rng(3), (T, nr))
    d_y = ctx.to_device(x)
    job = (pkg._lib.RxFrontendJob * 1)(pkg._lib.RxFrontendJob(d_y.ptr, None, 1.0, 1.0, NT, 0))
    lib, h = ctx.lib, ctx.handle

    def refused(status):
        msg = (lib.isac_last_error(h) or b"").decode()
        assert status == 1 and "rx front end" in msg, (status, msg)         # ISAC_ERR_INVALID_ARG with a message

    for mode in (PHILOX_SPECTRAL, INJECTED_SPECTRAL, 9, -1):
        refused(front_end(ctx, d_y, 1.0, 1.0, NT, mode))
    refused(front_end(ctx, d_y, 1.0, 1.0, NT, INJECTED))                    # injected mode without a buffer
    refused(lib.isac_rx_frontend_batch_dev(h, job, C.c_int32(1), C.c_int64(T), C.c_int32(0), C.c_int32(NONE)))
    refused(lib.isac_rx_frontend_batch_dev(h, job, C.c_int32(1), C.c_int64(T), C.c_int32(-2), C.c_int32(NONE)))
    refused(lib.isac_rx_frontend_batch_dev(h, job, C.c_int32(0), C.c_int64(T), C.c_int32(nr), C.c_int32(NONE)))
    refused(lib.isac_rx_frontend_batch_dev(h, job, C.c_int32(-1), C.c_int64(T), C.c_int32(nr), C.c_int32(NONE)))
    refused(lib.isac_rx_frontend_batch_dev(h, None, C.c_int32(1), C.c_int64(T), C.c_int32(nr), C.c_int32(NONE)))
    refused(lib.isac_rx_frontend_batch_dev(h, job, C.c_int32(1), C.c_int64(0), C.c_int32(nr), C.c_int32(NONE)))
    refused(front_end(ctx, d_y, 1.0, 1.0, -1.0, NONE))                      # negative noise power
    with pytest.raises(pkg.IsacError):
        ctx.check(front_end(ctx, d_y, 1.0, 1.0, NT, PHILOX_SPECTRAL))
    assert np.array_equal(d_y.numpy(), x)                                   # nothing was written
    ctx.check(front_end(ctx, d_y, S1, S2, NT, NONE))                        # ... and the context is usable afterwards
    assert rel(d_y.numpy(), (x * S1) * S2) < RTOL


def test_mex_gateway_front_end_commands(tmp_path):
    """tests/_build/mex_frontend_host: 'pathLoss', 'thermalNoisePower', 'rxFrontEnd' (MATLAB array in / out and device handle in place, MATLAB's randn as injected
    noise) with MATLAB-shaped arguments, against the restatement at the bounds of the tests above and of tests/test_rx_frontend_cpu.py."""
    exe = os.path.join(ROOT, "tests", "_build", "mex_frontend_host")
    if not os.path.exists(exe):
        import __graft_entry__ as g
        g.build_mex_frontend_host()
    T, nr, fc = 6001, 2, 3.5e9
    rng = np.random.default_rng(42)
    y, w = cplx(rng, (T, nr)), cplx(rng, (T, nr))
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("<2q12d", T, nr, PL_DB, GAIN_DB, 290.0, 7.0, FS, fc, *UE_POS, *GNB_POS))       # the downlink order: the UE's own position first
        f.write(y.tobytes(order="F"))
        f.write(w.tobytes(order="F"))
    r = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split()[-2:] == ["isac:INVALID_ARG", "isac:INVALID_ARG"]
    buf = open(fout, "rb").read()
    pls = np.frombuffer(buf, dtype=np.float64, count=20)
    k = 0
    for sc in R.SCENARIOS:
        for los in (1, 0):
            assert abs(pls[k] - R.path_loss_38901(sc, fc, los, UE_POS, GNB_POS)) <= 1e-12, (sc, los)
            k += 1
    assert abs(pls[18] - R.fspl(fc, UE_POS, GNB_POS)) <= 1e-12
    assert abs(pls[19] - NT) <= math.ulp(NT)
    arrs = np.frombuffer(buf, dtype=np.complex128, offset=160).reshape((T, nr, 3), order="F")
    want = R.rx_frontend(y, PL_DB, GAIN_DB, NT, w)
    assert rel(arrs[:, :, 0], want) < RTOL and rel(arrs[:, :, 1], want) < RTOL
    assert np.array_equal(arrs[:, :, 0], arrs[:, :, 1])
    assert rel(arrs[:, :, 2], R.rx_frontend(y, PL_DB, GAIN_DB, NT, None)) < RTOL
