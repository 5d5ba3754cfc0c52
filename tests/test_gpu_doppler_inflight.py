"""doppler_fft256_kernel (csrc/rdm.hip) with its loads in flight: every thread loads its own slow-time samples straight into the registers of the first radix-16 pass (no
staging slab), the two planes of the exchange go through one image of doubles, and a window whose bins all lie among the outputs k2 = 0 and 15 of the second pass
(bins -16 .. 15: the default CFAR area) takes an instantiation that forms only those.

isac_fft2d_get_power_window against the long-double restatement (tests/_transform_reference.py) with the rule tests/test_gpu_transforms.py uses for this kernel --
max |got - ref| <= 32 max(e_ref, 4 eps rms), e_ref the fp64 oracle's own distance from the reference -- at
  window rows nr in {9, 17, 40}     no multiple of the 16 rows of a workgroup: a partial last workgroup, one workgroup of 9, three of 40;
  L in {14, 28, 224, 256, 280}      zero padding (one load per thread, two, fourteen), the exact length, truncation (L > nFFT: the half-rotation wraps at L, not at 256);
  A in {1, 4}
and two detection areas each: one centred (window columns 114 .. 142, bins -14 .. 14: the pruned instantiation) and one wide and off-centre (columns 96 .. 172: the full
one).  The centred window is a block of the wide one, and the two instantiations must agree on it bit for bit.  nIFFT = 64 keeps the range stage and the reference small;
the Doppler kernel sees the range rows only."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import _transform_reference as R
import oracle as O
from conftest import load_pkg

pytestmark = pytest.mark.gpu

OK, NO_DETECTION = 0, 4
N_IFFT, K, N_FFT = 64, 48, 256
ROWS = {9: (10, 12), 17: (20, 30), 40: (4, 37)}           # CUT rows (1-based, inclusive) -> window rows nr = CUT rows + 2 (guard + training)
CENTRE, WIDE = (118, 140), (100, 170)                      # CUT columns (1-based, inclusive)


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context()
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _grids(L, A):
    """(rx, tx, the long-double map [nIFFT x nFFT x A], the fp64 oracle's) of a shape: computed once, never modified."""
    c = dict(K=K, L=L, A=A, n_fft=N_FFT, zero=None)
    rx, tx = R.plane_inputs(c, seed=41)
    rows = np.arange(N_IFFT)
    ref = np.stack([R.rdm_plane(rx[:, :, a], tx[:, :, a], N_IFFT, N_FFT, rows) for a in range(A)], axis=2)
    o64 = O.rdm_explicit(rx, tx, N_IFFT, N_FFT)
    for v in (rx, tx, ref, o64):
        v.setflags(write=False)
    return rx, tx, ref, o64


def _window(pkg, ctx, c, d_rx, d_tx):
    lib = ctx.lib
    ep = pkg._lib.EstParams(N_IFFT, N_FFT, 1.0, 1.0, 0, 0, 0, 360.0, 1.0, 180.0, 1.0)
    cf = pkg._lib.CfarConfig(R.PFA, (C.c_int32 * 2)(*R.GUARD), (C.c_int32 * 2)(*R.TRAIN), c["rows"][0], c["rows"][1], c["cols"][0], c["cols"][1])
    res = pkg._lib.EstResult()
    st = lib.isac_fft2d_dev(ctx.handle, C.byref(ep), C.byref(cf), d_rx, d_tx, K, c["L"], c["A"], C.byref(res))
    assert st in (OK, NO_DETECTION), (st, lib.isac_last_error(ctx.handle))
    dims, fr, fc = (C.c_int32 * 3)(), C.c_int32(0), C.c_int32(0)
    ctx.check(lib.isac_fft2d_get_power_window(ctx.handle, None, 0, dims, C.byref(fr), C.byref(fc)))
    r_lo, nr, c_lo, nc = R.window_geometry(c)
    assert tuple(dims) == (nr, nc, c["A"]) and (fr.value, fc.value) == (r_lo + 1, c_lo + 1)
    pwin = np.zeros(tuple(dims), dtype=np.float64, order="F")
    ctx.check(lib.isac_fft2d_get_power_window(ctx.handle, pwin.ctypes.data_as(C.c_void_p), pwin.size, dims, C.byref(fr), C.byref(fc)))
    return pwin


def _k2_set(c):
    """The outputs k2 of the second radix-16 pass a window's columns need (column <-> bin (column + 128) mod 256 = k1 + 16 k2)."""
    _, _, c_lo, nc = R.window_geometry(c)
    return {((col + N_FFT // 2) % N_FFT) >> 4 for col in range(c_lo, c_lo + nc)}


@pytest.mark.parametrize("A", [1, 4])
@pytest.mark.parametrize("L", [14, 28, 224, 256, 280])
@pytest.mark.parametrize("nr", [9, 17, 40])
def test_power_window_of_the_inflight_doppler_kernel(pkg, ctx, nr, L, A, record_property):
    rx, tx, ref_c, o64_c = _grids(L, A)
    d_rx, d_tx = ctx.to_device(rx), ctx.to_device(tx)
    got = {}
    try:
        for name, cols in (("centre", CENTRE), ("wide", WIDE)):
            c = dict(L=L, A=A, rows=ROWS[nr], cols=cols)
            r_lo, n_rows, c_lo, nc = R.window_geometry(c)
            assert n_rows == nr and n_rows % 16 != 0
            assert (_k2_set(c) <= {0, 15}) == (name == "centre"), "the centred window takes the pruned instantiation, the wide one the full"
            pwin = _window(pkg, ctx, c, d_rx, d_tx)
            ref = np.abs(ref_c[r_lo:r_lo + nr, c_lo:c_lo + nc]) ** 2
            o64 = np.abs(o64_c[r_lo:r_lo + nr, c_lo:c_lo + nc]) ** 2

            def report(m, name=name):
                ratio = m.err / m.e_ref if m.e_ref > 0 else float("inf")
                record_property(f"{name} err/rms", m.err / m.rms)
                print(f"DOPPLER nr {nr} L {L} A {A} {name}: e_ref/rms {m.e_ref / m.rms:.3e}  err/rms {m.err / m.rms:.3e}  ratio {ratio:.2f}  worst {m.idx}")

            R.check(pwin, ref, o64, report)
            got[name] = (c_lo, nc, pwin)
    finally:
        d_rx.free()
        d_tx.free()
    (c_lo, nc, centre), (w_lo, _, wide) = got["centre"], got["wide"]
    block = np.ascontiguousarray(wide[:, c_lo - w_lo:c_lo - w_lo + nc])
    assert block.shape == centre.shape and block.tobytes() == np.ascontiguousarray(centre).tobytes(), "the pruned and the full instantiation differ on a window both serve"
