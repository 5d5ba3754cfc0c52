"""The range stage, the Doppler kernels and the OFDM modulator / demodulator at every dispatched length, value by value against the long-double restatement
(tests/_transform_reference.py), through the transform entries of the C ABI with hand-made parameter blocks -- no physical scene:

  (a) isac_rdm_plane_dev: range_kernel<FFT> with every row + doppler_full_kernel, nIFFT = 64 ... 4096, and a second call of another shape on the same context;
  (b) the power window of fft2D: range_kernel on the CUT rows (the pruned one-block last pass of Fft4096W included), doppler_pow_kernel and
      doppler_fft256_kernel, isac_fft2d_get_power_window, with ISAC_OPT_TAIL_FUSION on and off;
  (c) isac_ofdm_modulate_dev, isac_ofdm_modulate_windowed_dev and isac_ofdm_demodulate_dev at Nfft = 128 ... 4096 and 15 / 30 / 60 / 120 kHz;
  (d) the host-side refusals of the two range entries and of a carrier below Nfft = 128.

Inputs are noise-like (complex normal rx, unit-modulus QPSK tx), so every output cell has a comparable magnitude and the rule of _transform_reference.check --
max |got - ref| <= 32 max(e_ref, 4 eps rms), e_ref the fp64 oracle's own distance from the reference -- sees a cell that is wrong by 1e-12 of the rms.
Each comparison records e_ref / rms, max |got - ref| / rms and their ratio (record_property; also printed)."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import _transform_reference as R
import oracle as O
from conftest import load_pkg

pytestmark = pytest.mark.gpu

OK, INVALID_ARG, NO_DETECTION, UNSUPPORTED = 0, 1, 4, 7


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture()
def ctx(pkg):
    c = pkg.Context()
    yield c
    c.close()


def _ep(pkg, n_ifft, n_fft):
    return pkg._lib.EstParams(n_ifft, n_fft, 1.0, 1.0, 0, 0, 0, 360.0, 1.0, 180.0, 1.0)


def _cfar(pkg, rows, cols):
    return pkg._lib.CfarConfig(R.PFA, (C.c_int32 * 2)(*R.GUARD), (C.c_int32 * 2)(*R.TRAIN), rows[0], rows[1], cols[0], cols[1])


def _report(record_property, label):
    def rep(m):
        ratio = m.err / m.e_ref if m.e_ref > 0 else float("inf")
        for k, v in (("e_ref/rms", m.e_ref / m.rms), ("err/rms", m.err / m.rms), ("ratio", ratio)):
            record_property(f"{label} {k}", v)
        print(f"TRANSFORM {label}: e_ref/rms {m.e_ref / m.rms:.3e}  err/rms {m.err / m.rms:.3e}  ratio {ratio:.2f}  worst {m.idx}")
    return rep


def _noise_like(ref):
    a = np.abs(ref)
    assert float(a.max()) < 8 * float(np.sqrt(np.mean(a * a)))


# ------------------------------------------------------------------ (a) the full plane
@functools.lru_cache(maxsize=None)
def _plane_case(i):
    """Inputs, the reference and the oracle of PLANE_CASES[i] on the case's rows: computed once, never modified."""
    c = R.PLANE_CASES[i]
    rx, tx = R.plane_inputs(c)
    rows, a = R.plane_rows(c), c["ant"]
    ref = R.rdm_plane(rx[:, :, a], tx[:, :, a], c["n_ifft"], c["n_fft"], rows)
    o64 = O.rdm_explicit(rx, tx, c["n_ifft"], c["n_fft"])[rows, :, a]
    for v in (rx, tx, ref, o64):
        v.setflags(write=False)
    return c, rx, tx, rows, ref, o64


def _rdm_plane(pkg, ctx, c, rx, tx, ant=None):
    d_rx, d_tx = ctx.to_device(rx), ctx.to_device(tx)
    d_out = ctx.empty((c["n_ifft"], c["n_fft"]))
    ep = _ep(pkg, c["n_ifft"], c["n_fft"])
    ctx.check(ctx.lib.isac_rdm_plane_dev(ctx.handle, C.byref(ep), d_rx, d_tx, c["K"], c["L"], c["A"], c["ant"] if ant is None else ant, d_out))
    out = d_out.numpy()
    for d in (d_rx, d_tx, d_out):
        d.free()
    return out


_FIRST_CALL = {}


def _plane_on_a_fresh_context(pkg, i):
    """The plane of case i as the first call of a context (kept: the order test of every case compares with its neighbour's)."""
    if i not in _FIRST_CALL:
        c, rx, tx = _plane_case(i)[:3]
        ctx = pkg.Context()
        try:
            _FIRST_CALL[i] = _rdm_plane(pkg, ctx, c, rx, tx)
        finally:
            ctx.close()
    return _FIRST_CALL[i]


@pytest.mark.parametrize("i", range(len(R.PLANE_CASES)), ids=[R.case_id(c) for c in R.PLANE_CASES])
def test_rdm_plane(pkg, ctx, i, record_property):
    c, rx, tx, rows, ref, o64 = _plane_case(i)
    _noise_like(ref)
    got = _rdm_plane(pkg, ctx, c, rx, tx)
    assert got.shape == (c["n_ifft"], c["n_fft"])
    R.check(got[rows], ref, o64, _report(record_property, "plane " + R.case_id(c)))
    if c["zero"]:                                           # the same case with every tx symbol silent: range_kernel's early exit on all columns
        z = _rdm_plane(pkg, ctx, c, rx, np.zeros_like(tx))
        assert not z.any()
    # the order of the calls on a context does not matter (stage_a and the cached tables are reused across sizes): `got` was this context's first call; the
    # next case's shape behind it gives what it gives as the first call of a context of its own, and this case once more, behind that, gives `got`
    assert np.array_equal(got, _FIRST_CALL.setdefault(i, got))
    j = (i + 1) % len(R.PLANE_CASES)
    cj, rxj, txj = _plane_case(j)[:3]
    assert np.array_equal(_rdm_plane(pkg, ctx, cj, rxj, txj), _plane_on_a_fresh_context(pkg, j))
    assert np.array_equal(_rdm_plane(pkg, ctx, c, rx, tx), got)


# ------------------------------------------------------------------ (b) the power window of fft2D
def _power_window(pkg, ctx, c, d_rx, d_tx):
    """(status, power window [nr x nc x A], total detections) of one fft2D call on the case's grids."""
    lib = ctx.lib
    ep, cf, res = _ep(pkg, c["n_ifft"], c["n_fft"]), _cfar(pkg, c["rows"], c["cols"]), pkg._lib.EstResult()
    st = lib.isac_fft2d_dev(ctx.handle, C.byref(ep), C.byref(cf), d_rx, d_tx, c["K"], c["L"], c["A"], C.byref(res))
    dims, fr, fc = (C.c_int32 * 3)(), C.c_int32(0), C.c_int32(0)
    ctx.check(lib.isac_fft2d_get_power_window(ctx.handle, None, 0, dims, C.byref(fr), C.byref(fc)))
    r_lo, nr, c_lo, nc = R.window_geometry(c)
    assert tuple(dims) == (nr, nc, c["A"]) and (fr.value, fc.value) == (r_lo + 1, c_lo + 1)
    pwin = np.zeros(tuple(dims), dtype=np.float64, order="F")
    ctx.check(lib.isac_fft2d_get_power_window(ctx.handle, pwin.ctypes.data_as(C.c_void_p), pwin.size, dims, C.byref(fr), C.byref(fc)))
    return st, pwin, int(res.total_detections)


@pytest.mark.parametrize("c", R.WINDOW_CASES, ids=R.case_id)
def test_fft2d_power_window(pkg, ctx, c, record_property):
    rx, tx, amp, added = R.window_inputs(c)
    assert added < 0.10                                     # the planted tone adds less than 10 % to the grid's energy
    r_lo, nr, c_lo, nc = R.window_geometry(c)
    rows = np.arange(r_lo, r_lo + nr)
    full = O.rdm_explicit(rx, tx, c["n_ifft"], c["n_fft"])
    ref_c = np.stack([R.rdm_plane(rx[:, :, a], tx[:, :, a], c["n_ifft"], c["n_fft"], rows) for a in range(c["A"])], axis=2)
    ref, o64 = np.abs(ref_c[:, c_lo:c_lo + nc]) ** 2, np.abs(full[r_lo:r_lo + nr, c_lo:c_lo + nc]) ** 2
    # ... and its cell, a CUT, stands about 50 times over the floor: sum w_k^2 Lu w_r[row]^2 / (nIFFT nFFT) at its row for unit-variance noise
    tr, tc = c["r0"], (c["d0"] + c["n_fft"] // 2) % c["n_fft"]
    assert c["rows"][0] <= tr + 1 <= c["rows"][1] and c["cols"][0] <= tc + 1 <= c["cols"][1]
    wk, wr = R.kaiser(c["K"], 3), R.kaiser(c["n_ifft"], 3)[R.fftshift_index(c["n_ifft"])]
    floor = float((wk * wk).sum() * min(c["L"], c["n_fft"]) * wr[tr] ** 2) / (c["n_ifft"] * c["n_fft"])
    assert all(20 < float(ref[tr - r_lo, tc - c_lo, a]) / floor < 100 for a in range(c["A"]))
    # what fft2D answers: the oracle's detector on the oracle's map of the same grids (a tone whose zero-padded main lobe covers the one-cell training ring
    # raises its own threshold: no detection, and the reference's findpeaks error)
    cc, rr = np.meshgrid(np.arange(c["cols"][0], c["cols"][1] + 1), np.arange(c["rows"][0], c["rows"][1] + 1))
    cut = np.stack([rr.ravel(order="F"), cc.ravel(order="F")])
    n_det = sum(O.ca_cfar2d(np.abs(full[:, :, a]) ** 2, cut, R.PFA, R.GUARD, R.TRAIN).shape[1] for a in range(c["A"]))
    d_rx, d_tx = ctx.to_device(rx), ctx.to_device(tx)
    windows = []
    for fusion in (True, False):
        ctx.set_tail_fusion(fusion)
        st, pwin, total = _power_window(pkg, ctx, c, d_rx, d_tx)
        assert st == (OK if n_det else NO_DETECTION), (st, ctx.lib.isac_last_error(ctx.handle))
        assert total == n_det
        windows.append(pwin)
    R.check(windows[0], ref, o64, _report(record_property, "window " + R.case_id(c)))
    assert np.array_equal(windows[0], windows[1])           # ISAC_OPT_TAIL_FUSION changes the detector only
    if c["n_ifft"] == 4096:                                 # the same rows through the full last pass of every row: pruned and full against one reference
        a = c["A"] - 1
        pc = dict(c, ant=a)
        plane = _rdm_plane(pkg, ctx, pc, rx, tx)
        R.check(plane[rows], ref_c[:, :, a], full[rows, :, a], _report(record_property, "window-rows-of-plane " + R.case_id(c)))


# ------------------------------------------------------------------ (c) OFDM
def _carrier(pkg, c):
    return pkg._lib.Carrier(c["n_sc"], c["nfft"], c["scs"], 0)


def _modulate(pkg, ctx, c, grid, t, n_slot=None, windowing=0):
    d_grid, d_wave = ctx.to_device(grid), ctx.empty((t, c["A"]))
    car = _carrier(pkg, c)
    if n_slot is None:
        st = ctx.lib.isac_ofdm_modulate_dev(ctx.handle, d_grid, c["L"], c["A"], C.byref(car), 1.0, d_wave, t)
    else:
        st = ctx.lib.isac_ofdm_modulate_windowed_dev(ctx.handle, d_grid, c["L"], c["A"], C.byref(car), 1.0, n_slot, windowing, d_wave, t)
    ctx.check(st)
    return d_wave


def _demodulate(pkg, ctx, c, d_wave, t, n_cols):
    d_grid = ctx.empty((c["n_sc"], n_cols, c["A"]))
    car = _carrier(pkg, c)
    ctx.check(ctx.lib.isac_ofdm_demodulate_dev(ctx.handle, d_wave, t, c["A"], C.byref(car), d_grid, n_cols))
    return d_grid.numpy()


@pytest.mark.parametrize("c", R.OFDM_CASES, ids=R.case_id)
def test_ofdm_modulate_demodulate(pkg, ctx, c, record_property):
    grid, wave = R.ofdm_inputs(c)
    t = wave.shape[0]
    td_idx, rows = R.ofdm_subsets(c)
    label = "ofdm " + R.case_id(c)
    # modulator: QPSK grid -> waveform
    ref = R.ofdm_modulate(grid, c["nfft"], c["scs"], td_idx=td_idx)
    keep = np.isfinite(ref.real)
    o64 = O.ofdm_modulate(grid, c["nfft"], c["scs"])
    assert ref.shape == (t, c["A"])
    _noise_like(ref[keep])
    d_mod = _modulate(pkg, ctx, c, grid, t)
    got = d_mod.numpy()
    R.check(got[keep], ref[keep], o64[keep], _report(record_property, label + " modulate"))
    # demodulator: a noise-like waveform, so that every bin carries energy
    sel = slice(None) if rows is None else rows
    ref = R.ofdm_demodulate(wave, c["n_sc"], c["nfft"], c["scs"], rows)
    _noise_like(ref)
    got = _demodulate(pkg, ctx, c, ctx.to_device(wave), t, c["L"])
    R.check(got[sel], ref, O.ofdm_demodulate(wave, c["n_sc"], c["nfft"], c["scs"])[sel], _report(record_property, label + " demodulate"))
    # round trip on the device against the grid itself
    got = _demodulate(pkg, ctx, c, d_mod, t, c["L"])
    R.check(got, grid, O.ofdm_demodulate(o64, c["n_sc"], c["nfft"], c["scs"]), _report(record_property, label + " round-trip"))


@pytest.mark.parametrize("c", R.WINDOWED_CASES, ids=R.case_id)
def test_ofdm_modulate_windowed(pkg, ctx, c, record_property):
    first = (c["n_slot"] % (c["scs"] // 15)) * 14
    grid, wave = R.ofdm_inputs(c, first_symbol=first)
    ref = R.ofdm_modulate(grid, c["nfft"], c["scs"], c["windowing"], first)
    o64 = O.ofdm_modulate(grid, c["nfft"], c["scs"], c["windowing"], first)
    got = _modulate(pkg, ctx, c, grid, wave.shape[0], c["n_slot"], c["windowing"]).numpy()
    R.check(got, ref, o64, _report(record_property, "ofdm-windowed " + R.case_id(c)))


@pytest.mark.parametrize("c", R.WINDOWED_CASES, ids=R.case_id)
def test_ofdm_demodulate_partial_last_symbol(pkg, ctx, c, record_property):
    """A waveform seven samples short of its last symbol holds L - 1 whole ones; the grid's last column stays zero."""
    _, wave = R.ofdm_inputs(c)
    wave = np.asfortranarray(wave[:-7])
    t = wave.shape[0]
    n = C.c_int32(0)
    car = _carrier(pkg, c)
    assert ctx.lib.isac_ofdm_symbol_count(C.byref(car), t, C.byref(n)) == OK and n.value == c["L"] - 1
    ref = R.ofdm_demodulate(wave, c["n_sc"], c["nfft"], c["scs"])
    assert ref.shape[1] == c["L"] - 1
    got = _demodulate(pkg, ctx, c, ctx.to_device(wave), t, c["L"])
    R.check(got[:, :-1], ref, O.ofdm_demodulate(wave, c["n_sc"], c["nfft"], c["scs"]), _report(record_property, "ofdm-partial " + R.case_id(c)))
    assert not got[:, -1].any()


# ------------------------------------------------------------------ (d) refusals: host-side returns before any launch
def test_range_entries_refuse_bad_dimensions(pkg, ctx):
    lib = ctx.lib
    c = R.PLANE_CASES[0]                                    # K 48, nIFFT 64, L 7, nFFT 16
    rx, tx = R.plane_inputs(c)
    d_rx, d_tx, d_out = ctx.to_device(rx), ctx.to_device(tx), ctx.empty((64, 16))
    want = _plane_case(0)

    def stage(n_ifft=64, n_fft=16, K=48, L=7, A=1, rows=(4, 61)):
        ep, cf = _ep(pkg, n_ifft, n_fft), _cfar(pkg, rows, (4, 13))
        return lib.isac_fft2d_range_stage_dev(ctx.handle, C.byref(ep), C.byref(cf), d_rx, d_tx, K, L, A)

    def plane(n_ifft=64, n_fft=16, K=48, L=7, A=1, ant=0):
        ep = _ep(pkg, n_ifft, n_fft)
        return lib.isac_rdm_plane_dev(ctx.handle, C.byref(ep), d_rx, d_tx, K, L, A, ant, d_out)

    def still_works():
        assert stage() == OK and plane() == OK
        R.check(d_out.numpy()[want[3]], want[4], want[5])

    still_works()
    bad = [dict(K=0), dict(K=-3), dict(L=0), dict(L=-1), dict(A=0), dict(A=-2), dict(n_ifft=32), dict(n_ifft=96), dict(n_fft=0), dict(n_fft=-16), dict(n_fft=12)]
    for entry in (stage, plane):
        for kw in bad:
            assert entry(**kw) == INVALID_ARG, (entry.__name__, kw)
            assert lib.isac_last_error(ctx.handle)
            still_works()
    for ant in (-1, 1):
        assert plane(ant=ant) == INVALID_ARG
        still_works()
    # a power of two outside 64 ... 4096 is a length the library does not have, not a malformed call
    for call in (lambda: stage(n_ifft=32, K=16, rows=(4, 20)), lambda: plane(n_ifft=32, K=16), lambda: stage(n_ifft=8192), lambda: plane(n_ifft=8192)):
        assert call() == UNSUPPORTED
        still_works()


def test_ofdm_entries_refuse_a_carrier_below_128_points(pkg, ctx):
    """No integral normal-CP length exists at Nfft = 64 (9 Nfft / 128 = 4.5 samples); nrOFDMInfo's minimum is 128."""
    lib = ctx.lib
    ok = R.OFDM_CASES[0]
    grid, wave = R.ofdm_inputs(ok)
    t = wave.shape[0]
    d_grid, d_wave = ctx.to_device(grid), ctx.to_device(wave)
    small = pkg._lib.Carrier(48, 64, 30, 0)
    car = _carrier(pkg, ok)
    calls = [lambda k: lib.isac_ofdm_demodulate_dev(ctx.handle, d_wave, t, ok["A"], C.byref(k), d_grid, ok["L"]),
             lambda k: lib.isac_ofdm_modulate_dev(ctx.handle, d_grid, ok["L"], ok["A"], C.byref(k), 1.0, d_wave, t),
             lambda k: lib.isac_ofdm_modulate_windowed_dev(ctx.handle, d_grid, ok["L"], ok["A"], C.byref(k), 1.0, 0, 4, d_wave, t)]
    for call in calls:
        assert call(small) == UNSUPPORTED
        assert b"128" in lib.isac_last_error(ctx.handle)
        assert call(car) == OK
    ctx.sync()
