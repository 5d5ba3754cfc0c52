"""Multi-static echo synthesis on the device (project-defined: include/isac_multistatic.h; csrc/multistatic.hip path_coef_kernel + echo.hip's tails).

RTOL = 1e-10 relative to the field's maximum, the project's bound for complex fp64 fields (test_gpu_parity.py, test_gpu_numerology.py); every comparison prints what it measured.
  1. against tests/_multistatic_restatement.py: waveform and grid, noise NONE / INJECTED, INJECTED_SPECTRAL against sum_p a_p D_p + W; shapes at the kernel's edges
  2. mono-static path lists: bit for bit isac_mono_static_sensing_dev (five noise modes) and isac_basic_radar_channel_dev
  3. the Philox field does not depend on the paths: (seeded - noiseless) equals the mono-static call's difference
  4. the three physical scenes end to end: multiStaticPaths -> multiStaticSensing -> fft2D against the oracle on the restatement's grid
  5. refusals: status, and a poison-filled output left untouched
The carriers are the two smallest of the numerology table (Nfft 256, 56 symbols) and scs60_nrb24_a4 for the physical scenes."""
from __future__ import annotations

import ctypes as C
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest

import oracle as O
import _multistatic_restatement as M
import _numerology_scenes as N
from conftest import load_pkg

pytestmark = pytest.mark.gpu
RTOL = 1e-10
MARGIN = 1e-6
FC = 3.5e9
CUT = 37                                                                    # samples taken off the waveform: T is no multiple of 256 and the last symbol is incomplete


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


def _bits(x):
    return np.ascontiguousarray(np.asarray(x).ravel(order="K")).view(np.uint64)


def _cnormal(rng, shape):
    return np.asfortranarray(rng.standard_normal(shape) + 1j * rng.standard_normal(shape))


# ---------------------------------------------------------------- 1. against the restatement
A_SRC = (2, 5, 8)
# name -> (carrier of the numerology table, receive elements, paths per source, sources without a waveform)
EDGE_CASES = {
    "p1_one_source": ("scs60_nrb11_a2", 2, (0, 1, 0), (0, 2)),              # all paths on one source; the other two pointers NULL
    "p2": ("scs120_nrb11_a2", 4, (1, 0, 1), (1,)),
    "p3": ("scs60_nrb11_a2", 4, (1, 1, 1), ()),
    "p8_full_tile": ("scs120_nrb11_a2", 2, (0, 0, 8), (0,)),
    "p9_one_over": ("scs60_nrb11_a2", 2, (0, 9, 0), ()),                    # sources 0 and 2 have waveforms that no path names
    "p17_two_tiles_and_one": ("scs120_nrb11_a2", 4, (9, 3, 5), ()),
}
_edge = {}


def _edge_case(name):
    """namespace(case, T, waves, rp, paths, rows, noise, wave0, wave1, grid0, grid1): random source waveforms of the carrier's length less CUT samples, random paths -- unit
    steering phases, gains around 1, Doppler of both signs, shifts 0 / equal on two sources / beyond a symbol / T - 1 / >= T -- and the restatement's results without noise and
    with the injected time-domain noise (N0 = 2: unit noise, about the size of the signal).  Made once per process."""
    if name in _edge:
        return _edge[name]
    cname, A, per_source, absent = EDGE_CASES[name]
    case = N.CASE[cname]
    nfft, scs, K = case.nfft, case.scs, 12 * case.nrb
    T = int(O.symbol_starts(nfft, scs, case.L + 1)[0][case.L]) - CUT
    rng = np.random.default_rng(sum(per_source) * 100 + A)
    waves = [None if s in absent else _cnormal(rng, (T, A_SRC[s])) for s in range(3)]
    source = np.repeat(np.arange(3), per_source).astype(np.int32)
    rng.shuffle(source)                                                     # input order is not source order
    P = source.size
    specials = [0, 0, nfft + 2 * case.cp[1] + 5, T - 1, T, T + 1000, 3, 3]  # 0; beyond one symbol; T - 1; >= T; equal shifts (3) land on two sources where there are two
    shift = np.array([specials[p] if p < len(specials) else int(rng.integers(0, 4 * nfft)) for p in range(P)], dtype=np.int64)
    if P < 4:
        shift = np.array([0, nfft + 2 * case.cp[1] + 5, 7][:P], dtype=np.int64)
    doppler = rng.uniform(-4e3, 4e3, P)
    doppler[0] = -abs(doppler[0])
    if P > 1:
        doppler[1] = abs(doppler[1])
    gain = rng.uniform(0.5, 1.5, P)
    tx_st = [np.exp(2j * np.pi * rng.random(A_SRC[s])) for s in source]
    rx_st = np.asfortranarray(np.exp(2j * np.pi * rng.random((A, P))))
    paths = SimpleNamespace(source=source, shift=shift, doppler=doppler, gain=gain, txSteering=tx_st, rxSteering=rx_st)
    rp = SimpleNamespace(fc=FC, fs=float(nfft * scs * 1e3), N0=2.0, nTxAnts=A)
    rows = M.path_tuples(paths)
    noise = _cnormal(rng, (T, A))
    ch = lambda nz: np.asfortranarray(M.multi_static_channel(waves, rp.fc, rp.fs, rp.N0, A, rows, nz))
    wave0, wave1 = ch(None), ch(noise)
    L_out = case.L + 2                                                      # two padded symbol columns behind the L - 1 whole symbols of the cut waveform
    dm = lambda w: np.asfortranarray(np.concatenate([O.ofdm_demodulate(w, K, nfft, scs), np.zeros((K, 3, A))], axis=1))
    v = SimpleNamespace(case=case, T=T, K=K, A=A, L_out=L_out, waves=waves, rp=rp, paths=paths, rows=rows, noise=noise, wave0=wave0, wave1=wave1, grid0=dm(wave0), grid1=dm(wave1),
                        carrier=SimpleNamespace(NRBsDL=case.nrb, SubcarrierSpacing=scs))
    for arr in [w for w in waves if w is not None] + [noise, wave0, wave1, v.grid0, v.grid1]:
        arr.setflags(write=False)
    _edge[name] = v
    return v


def test_edge_cases_reach_every_edge():
    seen_p, seen_a = set(), set()
    for name in EDGE_CASES:
        e = _edge_case(name)
        P = e.paths.source.size
        seen_p.add(P)
        seen_a.add(e.A)
        assert e.T % 256 != 0 and e.grid0.shape == (e.K, e.case.L + 2, e.A) and not e.grid0[:, e.case.L - 1:, :].any() and e.grid0[:, e.case.L - 2, :].any()
        assert (e.paths.doppler < 0).any() and (P == 1 or (e.paths.doppler > 0).any()) and 0 in e.paths.shift.tolist()
        if P >= 3:
            assert (e.paths.shift > e.case.nfft + e.case.cp[1]).any()
        if P >= 8:
            assert {e.T - 1, e.T, e.T + 1000} <= set(e.paths.shift.tolist())
    assert seen_p == {1, 2, 3, 8, 9, 17} and seen_a == {2, 4}
    big = _edge_case("p17_two_tiles_and_one")
    same = [(p, q) for p in range(17) for q in range(p) if big.paths.shift[p] == big.paths.shift[q] and big.paths.source[p] != big.paths.source[q]]
    assert same, "no two paths of different sources with equal shifts"
    counts = np.bincount(big.paths.source, minlength=3).tolist()
    assert counts == [9, 3, 5] and sorted(big.paths.source.tolist()) != big.paths.source.tolist()
    assert [w is None for w in _edge_case("p1_one_source").waves] == [True, False, True]
    assert all(w is not None for w in _edge_case("p9_one_over").waves) and set(_edge_case("p9_one_over").paths.source.tolist()) == {1}


@pytest.mark.parametrize("name", list(EDGE_CASES))
def test_waveform_and_grid_against_the_restatement(pkg, name):
    e = _edge_case(name)
    ctx = pkg.default_context()
    d_waves = [None if w is None else ctx.to_device(w) for w in e.waves]
    chan, sens = pkg.sensing.channelModels.multiStaticChannel, pkg.sensing.multiStaticSensing
    dims = (e.K, e.L_out, e.A)
    errs = {}
    errs["wave_none"] = N.rel(chan(d_waves, e.rp, e.paths).numpy(), e.wave0)
    errs["wave_injected"] = N.rel(chan(d_waves, e.rp, e.paths, noise=e.noise).numpy(), e.wave1)
    g0 = sens(d_waves, dims, e.carrier, e.rp, e.paths, nfft=e.case.nfft).numpy()
    g1 = sens(d_waves, dims, e.carrier, e.rp, e.paths, nfft=e.case.nfft, noise=ctx.to_device(e.noise)).numpy()
    errs["grid_none"], errs["grid_injected"] = N.rel(g0, e.grid0), N.rel(g1, e.grid1)
    # INJECTED_SPECTRAL: sum_p a_p D_p + sqrt(N0 / 2) sqrt(Nfft) W, D_p = OFDM-demodulate(coef_p) -- coef_p from the restatement with the path alone on one receive element
    rng = np.random.default_rng(7)
    W = _cnormal(rng, dims)
    want = np.zeros(dims, dtype=np.complex128, order="F")
    for (s, d, f, g, b, a) in e.rows:
        coef = M.multi_static_channel(e.waves, e.rp.fc, e.rp.fs, e.rp.N0, 1, [(s, d, f, g, b, np.ones(1))], None)
        D = O.ofdm_demodulate(coef, e.K, e.case.nfft, e.case.scs)
        want[:, :D.shape[1], :] += D * a[None, None, :]
    want += np.sqrt(e.rp.N0 / 2.0) * np.sqrt(e.case.nfft) * W
    want[:, e.case.L - 1:, :] = 0                                           # the padded columns hold no noise either
    gs = sens(d_waves, dims, e.carrier, e.rp, e.paths, nfft=e.case.nfft, spectral_noise=W).numpy()
    errs["grid_injected_spectral"] = N.rel(gs, want)
    gz = sens([None if w is None else np.asarray(w) for w in e.waves], dims, e.carrier, e.rp, e.paths, nfft=e.case.nfft, spectral_noise=np.zeros(dims))   # NumPy in, NumPy out
    errs["grid_spectral_no_noise"] = N.rel(gz, e.grid0)
    print(f"{name}: " + ", ".join(f"{k} {v:.3e}" for k, v in errs.items()))
    assert g0.shape == dims and isinstance(gz, np.ndarray) and not g1[:, e.case.L - 1:, :].any() and not gs[:, e.case.L - 1:, :].any()
    assert float(np.abs(e.wave1 - e.wave0).max()) > 0.1 * float(np.abs(e.wave0).max())          # the noise is there
    for k, v in errs.items():
        assert v <= RTOL, k


# ---------------------------------------------------------------- 2. mono-static identity
def _mono_scene(pkg, q):
    """scs60_nrb11_a2's shape with q targets (the third one NLoS where there are three or more): the table scene's waveform and noise, sensing.radarParams' record."""
    targets = tuple((90.0 + 35.0 * i, 20.0 - 11.0 * i, 1.5) for i in range(q))
    sc = N.scene(60, 11, 2, 4, targets, tuple(15.0 - 6.0 * i for i in range(q)), 6, False, seed=11 + q)
    rp = pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)
    los = np.ones(q, dtype=np.uint8)
    if q >= 3:
        los[2] = 0
    return sc, rp, los


@pytest.mark.parametrize("q", [1, 2, 3, 9])
def test_mono_static_paths_give_the_mono_static_bits(pkg, q):
    sc, rp, los = _mono_scene(pkg, q)
    paths = M.mono_static_paths(rp, los)
    assert len(paths.source) == int(los.sum())
    ctx = pkg.Context()
    try:
        d_wave, d_noise = ctx.to_device(sc.tx_wave), ctx.to_device(sc.noise)
        dims = (sc.K, sc.L + 1, sc.A)                                       # one padded column
        W = ctx.to_device(_cnormal(np.random.default_rng(q), dims))
        modes = dict(none={}, injected=dict(noise=d_noise), philox=dict(seed=77 + q), philox_spectral=dict(seed=99 + q, noise_domain="spectral"), injected_spectral=dict(spectral_noise=W))
        grids = {}
        for m, kw in modes.items():
            want = pkg.sensing.monoStaticSensing(d_wave, dims, sc.carrier, rp, los, nfft=sc.wave.Nfft, ctx=ctx, **kw).numpy()
            got = pkg.sensing.multiStaticSensing([d_wave], dims, sc.carrier, rp, paths, nfft=sc.wave.Nfft, ctx=ctx, **kw).numpy()
            assert got.shape == want.shape == dims and want[:, :sc.L, :].any() and not want[:, sc.L:, :].any()
            assert np.array_equal(_bits(got), _bits(want)), f"grid, noise mode {m}"
            grids[m] = want
        assert len({g.tobytes() for g in grids.values()}) == 5              # five different grids: the modes were really taken
        for m in ("none", "injected", "philox"):
            want = pkg.sensing.channelModels.basicRadarChannel(d_wave, rp, los, ctx=ctx, **modes[m]).numpy()
            got = pkg.sensing.channelModels.multiStaticChannel([d_wave], rp, paths, ctx=ctx, **modes[m]).numpy()
            assert want.any() and np.array_equal(_bits(got), _bits(want)), f"waveform, noise mode {m}"
    finally:
        ctx.close()


# ---------------------------------------------------------------- 3. the Philox field is a function of the seed and the receive grid only
@pytest.mark.parametrize("domain", ["time", "spectral"])
def test_philox_noise_does_not_depend_on_the_paths(pkg, domain):
    e = _edge_case("p17_two_tiles_and_one")
    sc, rp, los = _mono_scene(pkg, 2)
    ctx = pkg.default_context()
    T, dims = e.T, (e.K, e.L_out, e.A)
    rng = np.random.default_rng(3)
    own = ctx.to_device(_cnormal(rng, (T, e.A)))                             # a mono-static cell with the receive array, length, carrier and N0 of the edge case
    rp.nTxAnts, rp.N0, rp.fs = e.A, e.rp.N0, e.rp.fs
    rp.RxSteeringVec = np.exp(2j * np.pi * rng.random((e.A, 2)))
    rp.largeScaleFading = np.array([0.7, 1.1])
    kw = dict(nfft=e.case.nfft, ctx=ctx)
    seeded = dict(seed=0xC0FFEE, noise_domain=domain)
    mono = pkg.sensing.monoStaticSensing(own, dims, e.carrier, rp, los, **kw, **seeded).numpy() - pkg.sensing.monoStaticSensing(own, dims, e.carrier, rp, los, **kw).numpy()
    d_waves = [ctx.to_device(w) for w in e.waves]
    multi = pkg.sensing.multiStaticSensing(d_waves, dims, e.carrier, e.rp, e.paths, **kw, **seeded).numpy() - pkg.sensing.multiStaticSensing(d_waves, dims, e.carrier, e.rp, e.paths, **kw).numpy()
    rms = float(np.sqrt(np.mean(np.abs(mono[:, :e.case.L - 1, :]) ** 2)))
    err = float(np.abs(multi - mono).max()) / rms
    print(f"{domain}: noise rms {rms:.3e} (sqrt(N0 Nfft) = {np.sqrt(e.rp.N0 * e.case.nfft):.3e}), difference of the two noise fields {err:.3e} of it")
    assert 0.9 * np.sqrt(e.rp.N0 * e.case.nfft) < rms < 1.1 * np.sqrt(e.rp.N0 * e.case.nfft)
    assert err <= RTOL


# ---------------------------------------------------------------- 4. the three physical scenes, end to end
def _device_scene(pkg, ctx, name):
    b, kw = M.base(), M.SCENES[name]
    sc = b.sc
    rp = pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)
    paths = pkg.sensing.channelModels.multiStaticPaths(sc.cell, [sc.cell, b.nb.cell], b.targets, carrierInfo=sc.carrier, waveInfo=sc.wave, directLoS=[1, kw["direct_los"]],
                                                       directLossdB=kw["loss_db"])
    grid = pkg.sensing.multiStaticSensing([ctx.to_device(sc.tx_wave), ctx.to_device(b.nb.tx_wave)], sc.tx_grid.shape, sc.carrier, rp, paths, noise=ctx.to_device(sc.noise),
                                          nfft=sc.wave.Nfft, ctx=ctx)
    return sc, rp, grid


def _fft2d_against_the_oracle(pkg, ctx, rp, grid, tx_grid, want, what):
    est_o, dets_o, margin = want
    assert all(m > MARGIN for m in margin), f"{what}: a CUT cell lies within {min(margin):.2e} of its threshold"
    cf = pkg.sensing.detection.cfar2D(rp)
    try:
        est, dbg = pkg.sensing.estimation.fft2D(rp, cf, grid, ctx.to_device(tx_grid), return_debug=True, ctx=ctx)
    except pkg.IsacError as err:
        assert err.name == "NO_DETECTION", err
        est, dbg = None, import_module(pkg.__name__ + ".sensing.estimation.fft2D").fft2D_debug(ctx, grid.shape[2])
    print(f"{what}: guard margin {min(margin):.3f}; detections per antenna {[d.shape[1] for d in dbg.detections]}; rngEst {None if est is None else est.rngEst.tolist()}")
    assert len(dbg.detections) == len(dets_o)
    for a, (d, o) in enumerate(zip(dbg.detections, dets_o)):
        assert np.array_equal(d, o), f"{what}: antenna {a}"
    assert (est is None) == (est_o is None), f"{what}: ISAC_ERR_NO_DETECTION exactly where the oracle's findpeaks raises"
    if est is not None:
        assert np.array_equal(est.rngEst, est_o.rngEst) and np.array_equal(est.velEst, est_o.velEst) and np.array_equal(est.aziEst, est_o.aziEst), (est, est_o)
    return est


@pytest.mark.parametrize("name", list(M.SCENES))
def test_physical_scene_end_to_end(pkg, name):
    s, b = M.scene(name), M.base()
    ctx = pkg.Context()
    try:
        sc, rp, grid = _device_scene(pkg, ctx, name)
        err = N.rel(grid.numpy(), s.echo)
        print(f"{name}: echo grid against the restatement {err:.3e}")
        assert grid.shape == s.echo.shape and err <= RTOL
        own = _fft2d_against_the_oracle(pkg, ctx, rp, grid, sc.tx_grid, s.own, name + ", own grid")
        nbr = _fft2d_against_the_oracle(pkg, ctx, rp, grid, b.nb.tx_grid, s.nbr, name + ", neighbour's grid")
    finally:
        ctx.close()
    r_res = sc.rp.rRes
    if name == "bistatic":
        assert nbr.rngEst[0] == 44 * r_res and 44 * r_res not in own.rngEst.tolist() and own.rngEst[0] == 33 * r_res
    if name == "interference":
        assert own is None
    if name == "wall":
        assert own is not None and own.rngEst[0] == 33 * r_res


# ---------------------------------------------------------------- 5. refusals
def _refusal_args(T, A, P, S=2, a_src=(2, 3)):
    """Valid flat arrays for P paths spread over S sources; the caller breaks one thing."""
    rng = np.random.default_rng(5)
    a_src = np.asarray((a_src * 17)[:S], dtype=np.int32)
    source = (np.arange(P) % S).astype(np.int32)
    return SimpleNamespace(n_ants_src=a_src, source=source, shift=np.arange(P, dtype=np.int64), doppler=rng.uniform(-1e3, 1e3, P), gain=np.ones(P),
                           tx=np.exp(2j * np.pi * rng.random(int(a_src[source].sum()) if P else 1)), rx=np.exp(2j * np.pi * rng.random(max(A * P, 1))))


REFUSALS = {                                                                # name -> (status name, what to break)
    "no_path": ("NO_LOS", dict(P=0)),
    "source_index_too_large": ("INVALID_ARG", dict(source1=2)),
    "source_index_negative": ("INVALID_ARG", dict(source1=-1)),
    "negative_shift": ("INVALID_ARG", dict(shift1=-1)),
    "named_source_without_a_waveform": ("INVALID_ARG", dict(null_wave=1)),
    "too_many_paths": ("CAPACITY", dict(P=65)),
    "too_many_sources": ("CAPACITY", dict(S=33)),
    "too_many_receive_elements": ("CAPACITY", dict(A=257)),
    "too_many_source_elements": ("CAPACITY", dict(a_src=(2, 257))),
    "unknown_noise_mode": ("INVALID_ARG", dict(noise_mode=5)),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refused_calls_write_nothing(pkg, name):
    status, brk = REFUSALS[name]
    L = pkg._lib
    code = {v: k for k, v in L.STATUS_NAMES.items()}[status]
    case = N.CASE["scs60_nrb11_a2"]
    T = 2 * (case.nfft + case.cp[1]) + 50                                   # two whole symbols
    A, P, S, a_src = brk.get("A", 2), brk.get("P", 3), brk.get("S", 2), brk.get("a_src", (2, 3))
    v = _refusal_args(T, A, P, S, a_src)
    if "source1" in brk:
        v.source[1] = brk["source1"]
    if "shift1" in brk:
        v.shift[1] = brk["shift1"]
    ctx = pkg.Context()
    try:
        rng = np.random.default_rng(1)
        waves = [ctx.to_device(_cnormal(rng, (T, int(min(v.n_ants_src[s], 8))))) if s < 2 else None for s in range(S)]     # (a refused call reads no waveform)
        if "null_wave" in brk:
            waves[brk["null_wave"]] = None
        ptrs = (C.c_void_p * S)(*[None if w is None else w.ptr for w in waves])
        car = L.Carrier(12 * case.nrb, case.nfft, case.scs, 0)
        K, L_out = 12 * case.nrb, 3
        poison = np.float64(-7.25e300)
        p_ = lambda a: a.ctypes.data_as(C.c_void_p)
        args = (ctx.handle, ptrs, p_(v.n_ants_src), S, T, FC, float(case.nfft * case.scs * 1e3), 2.0, A, P, p_(v.source), p_(v.shift), p_(v.doppler), p_(v.gain), p_(v.tx), p_(v.rx),
                brk.get("noise_mode", L.NOISE_PHILOX), None, 12345)
        for call, shape, tail in (("isac_multi_static_channel_dev", (T, A), ()), ("isac_multi_static_sensing_dev", (K, L_out, A), None)):
            if call.endswith("channel_dev") and name == "unknown_noise_mode":
                args_c = args[:16] + (L.NOISE_PHILOX_SPECTRAL,) + args[17:]   # the channel call takes no spectral mode
            else:
                args_c = args
            out = ctx.to_device(np.full(shape, poison + 1j * poison, dtype=np.complex128, order="F"))
            lo = C.c_int32(-5)
            extra = (out,) if tail is not None else (L_out, C.byref(car), out, C.byref(lo))
            st = getattr(ctx.lib, call)(*args_c, *extra)
            ctx.sync()
            msg = (ctx.lib.isac_last_error(ctx.handle) or b"").decode()
            print(f"{name}, {call}: status {st} ({msg})")
            assert st == code, (call, st, msg)
            got = out.numpy()
            assert (got.real == poison).all() and (got.imag == poison).all(), f"{call}: a refused call wrote to its output"
            assert lo.value == -5
    finally:
        ctx.close()


def test_a_valid_call_of_the_refusal_shape_is_accepted(pkg):
    """The arrays the refusals start from, unbroken: ISAC_OK from both calls, so each refusal above is caused by what was broken."""
    L = pkg._lib
    case = N.CASE["scs60_nrb11_a2"]
    T = 2 * (case.nfft + case.cp[1]) + 50
    v = _refusal_args(T, 2, 3)
    ctx = pkg.Context()
    try:
        rng = np.random.default_rng(1)
        waves = [ctx.to_device(_cnormal(rng, (T, int(a)))) for a in v.n_ants_src]
        ptrs = (C.c_void_p * 2)(*[w.ptr for w in waves])
        car = L.Carrier(12 * case.nrb, case.nfft, case.scs, 0)
        p_ = lambda a: a.ctypes.data_as(C.c_void_p)
        args = (ctx.handle, ptrs, p_(v.n_ants_src), 2, T, FC, float(case.nfft * case.scs * 1e3), 2.0, 2, 3, p_(v.source), p_(v.shift), p_(v.doppler), p_(v.gain), p_(v.tx), p_(v.rx),
                L.NOISE_PHILOX, None, 12345)
        out_w, out_g, lo = ctx.empty((T, 2)), ctx.empty((12 * case.nrb, 3, 2)), C.c_int32(0)
        assert ctx.lib.isac_multi_static_channel_dev(*args, out_w) == 0
        assert ctx.lib.isac_multi_static_sensing_dev(*args, 3, C.byref(car), out_g, C.byref(lo)) == 0 and lo.value == 3
        g = out_g.numpy()
        assert out_w.numpy().any() and g[:, :2, :].any() and not g[:, 2:, :].any()
    finally:
        ctx.close()
