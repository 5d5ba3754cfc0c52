"""music2D's range and velocity pseudo-spectra (csrc/doa.hip isac_music2d_dev; csrc/music.hip chan_plane_kernel, signal_vectors_kernel,
music2d_scan_kernel) value by value: the device's dB spectra, read through music2D(..., return_debug=True) / Context.music2d_spectra(), against the
extended-precision reference of tests/_music2d_reference.py at TOL_DB = 1e-6 dB per scan point (the tolerance of the ULA and UPA maps); where the
reference lies above -200 dB both sides must be finite.  got.L is asserted first; rngEst / velEst must equal findpeaks on the DEVICE'S OWN spectra and
aziEst findpeaks on Context.angular_spectrum(), which separates the kernels from the host tail.

Shapes (K, Ls, A) by code path: (24, 14, 4) base; (12, 28, 4) K < Ls; 63 / 64 / 65 the first wave boundary and 255 / 256 / 257 the block boundary of the
256-thread strided sums; (48, 65, 4) a second wave in the velocity scan; (300, 14, 3) L = A - 1 with two targets one range step apart; (3276, 28, 4) the
named K.  One, two and three targets, an H-plane SNR of 10 and 30 dB everywhere and of 60 and 100 dB (targets on the 0.5 grids and off them) on three
shapes, L equal to the number of targets and one larger; L >= Ls (no velocity noise vector): flat 0 dB, no estimate.

tests/test_music2d_reference_cpu.py holds the cases' conditions (the fp64 statement of the reference's formulation within 1e-8 dB on every case here)
and shows that this comparison rejects twelve wrong kernels.  Largest deviations measured on an MI355X: DESIGN.md section 5."""
from __future__ import annotations

import copy
from types import SimpleNamespace

import numpy as np
import pytest

import _music2d_reference as M
import oracle as O
from conftest import load_pkg, make_scene

pytestmark = pytest.mark.gpu

TOL_DB = M.TOL_DB
WORST = {}              # (spectrum, case group) -> largest |device - reference| in dB
BS = SimpleNamespace(scs=M.SCS_KHZ)


@pytest.fixture(scope="module")
def pkg():
    return load_pkg()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context()
    yield c
    c.close()


def _peaks(spec, n):
    return O.findpeaks(spec, npeaks=n)[1]


def _run(pkg, ctx, c):
    """One music2D call; L first, then the host tail against the device's own spectra."""
    got, dbg = pkg.sensing.estimation.music2D(c.rp, BS, c.rx, c.tx, ctx=ctx, return_debug=True)
    assert got.L == c.L, (c.name, got.L)
    assert dbg.PrdB.size == c.r_grid.size and dbg.PvdB.size == c.v_grid.size
    assert np.array_equal(dbg.rGrid, c.r_grid) and np.array_equal(dbg.vGrid, c.v_grid)
    assert np.array_equal(got.rngEst, c.r_grid[_peaks(dbg.PrdB, got.L)]), (c.name, got.rngEst)
    assert np.array_equal(got.velEst, c.v_grid[_peaks(dbg.PvdB, got.L)]), (c.name, got.velEst)
    spec = ctx.angular_spectrum()
    assert spec.size == 361 and np.array_equal(got.aziEst, _peaks(spec, got.L) - 180.0) and np.all(np.isnan(got.eleEst))
    pr, pv = ctx.music2d_spectra()
    assert np.array_equal(pr, dbg.PrdB) and np.array_equal(pv, dbg.PvdB)
    return got, dbg


def _compare(dbg, ref, group, tag, record_property):
    for what, got, want in (("range", dbg.PrdB[ref.r_idx], ref.PrdB), ("velocity", dbg.PvdB[ref.v_idx], ref.PvdB)):
        d = M.deviation(got, want)
        print(f"{what} {group} {tag}: {d:.3e} dB")
        WORST[(what, group)] = max(WORST.get((what, group), 0.0), d)
        record_property(f"max_dev_db_{what}_{group}", WORST[(what, group)])
        assert d <= TOL_DB, (what, group, tag, d)


@pytest.mark.parametrize("group,args", M.ALL_CASES, ids=[f"{g}-{M.case_id(a)}" for g, a in M.ALL_CASES])
def test_spectra_against_the_reference(pkg, ctx, group, args, record_property):
    ref = M.reference(args)
    _, dbg = _run(pkg, ctx, ref.case)
    _compare(dbg, ref, group, M.case_id(args), record_property)


def test_empty_velocity_noise_space(pkg, ctx, record_property):
    """L = 2 >= Ls = 2: the reference divides by zero (NaN dB, no peak); the device: a flat 0 dB velocity spectrum and no velocity estimate (include/isac.h),
    the range spectrum as ever."""
    ref = M.reference(M.EMPTY_NOISE_SPACE)
    got, dbg = _run(pkg, ctx, ref.case)
    assert got.L >= ref.case.Ls
    assert np.all(dbg.PvdB == 0.0) and got.velEst.size == 0
    assert got.rngEst.size > 0
    _compare(dbg, ref, "empty", M.case_id(M.EMPTY_NOISE_SPACE), record_property)


def _no_spectra(pkg, ctx):
    with pytest.raises(pkg.IsacError) as ei:
        ctx.music2d_spectra()
    return ei.value.name == "INVALID_ARG"


def test_getter_contract(pkg):
    """isac_music2d_get_spectra hands out the spectra of the context's last completed music2D, and nothing else (include/isac.h)."""
    import ctypes as C
    music2d = pkg.sensing.estimation.music2D
    ctx = pkg.Context()
    assert _no_spectra(pkg, ctx)                                            # no music2D yet ...
    c8 = M.R.physical_case("a8")
    pkg.sensing.estimation.doaEstimation.music(2, M.R.rp_ula(n_ants=8), c8.ra, ctx=ctx)
    assert ctx.angular_spectrum().size == 361 and _no_spectra(pkg, ctx)     # ... and a stand-alone azimuth scan is none
    ref = M.reference(M.CASES["base"][0])
    c = ref.case
    music2d(c.rp, BS, c.rx, c.tx, ctx=ctx)
    # the lengths query, a short capacity, one spectrum at a time
    n = (C.c_int32 * 2)()
    ctx.check(ctx.lib.isac_music2d_get_spectra(ctx.handle, None, 0, None, 0, n))
    assert (n[0], n[1]) == (122, 122)
    pr, pv = np.full(122, 7.0), np.full(122, 7.0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                            # noqa: E731
    CAPACITY = {v: k for k, v in pkg._lib.STATUS_NAMES.items()}["CAPACITY"]
    assert ctx.lib.isac_music2d_get_spectra(ctx.handle, ptr(pr), 121, ptr(pv), 122, None) == CAPACITY
    assert ctx.lib.isac_music2d_get_spectra(ctx.handle, ptr(pr), 122, ptr(pv), 121, None) == CAPACITY
    assert np.all(pr == 7.0) and np.all(pv == 7.0)                          # nothing written
    ctx.check(ctx.lib.isac_music2d_get_spectra(ctx.handle, None, 0, ptr(pv), 122, None))
    assert np.all(pr == 7.0) and M.deviation(pv[ref.v_idx], ref.PvdB) <= TOL_DB
    ctx.check(ctx.lib.isac_music2d_get_spectra(ctx.handle, ptr(pr), 500, None, 0, n))
    assert M.deviation(pr[ref.r_idx], ref.PrdB) <= TOL_DB
    # a second music2D with another zone: its spectra, with its lengths
    rp2 = copy.copy(c.rp)
    rp2.cfarEstZone = np.array([[0.0, 40.0], [-20.0, 20.0]])
    _, dbg2 = music2d(rp2, BS, c.rx, c.tx, ctx=ctx, return_debug=True)
    assert dbg2.PrdB.size == 82 and dbg2.PvdB.size == 82 and dbg2.vGrid[0] == -20.0
    assert M.deviation(dbg2.PrdB[ref.r_idx[ref.r_idx < 82]], _renormalised(ref.PrdB[ref.r_idx < 82])) <= TOL_DB
    # other calls leave them alone
    pkg.sensing.estimation.doaEstimation.digitalBF(2, M.R.rp_ula(n_ants=8), c8.ra, ctx=ctx)
    assert np.array_equal(ctx.music2d_spectra()[0], dbg2.PrdB)
    # a music2D that fails (a UPA is refused) drops them
    rp_upa = copy.copy(c.rp)
    rp_upa.antennaType = SimpleNamespace(kind="upa", nV=2, nH=2)
    with pytest.raises(pkg.IsacError) as ei:
        music2d(rp_upa, BS, c.rx, c.tx, ctx=ctx)
    assert ei.value.name == "UNSUPPORTED" and _no_spectra(pkg, ctx)
    # ... and the next one brings them back
    music2d(c.rp, BS, c.rx, c.tx, ctx=ctx)
    assert M.deviation(ctx.music2d_spectra()[0][ref.r_idx], ref.PrdB) <= TOL_DB
    # isac_ctx_reserve's dry run re-plans the context: nothing from before it is handed out
    sc = make_scene(n_ants=8, n_slots=2, nrb=24, num_slots_param=3, zero_s_slots=False, seed=21, targets=((150.0, 40.0, 1.5),), velocity=(0.0,))
    rp = pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)
    pkg.sensing.reserve(sc.T, sc.tx_grid.shape, sc.carrier, rp, pkg.sensing.detection.cfar2D(rp), nfft=sc.wave.Nfft, ctx=ctx)
    assert _no_spectra(pkg, ctx)
    ctx.close()


def _renormalised(db):
    """A dB spectrum cut to its first points and normalised by ITS maximum (the first 82 range points of the 122: the same values of P)."""
    return db - db.max()


def test_zz_report():
    print("\nmusic2D spectra, largest |device - reference| in dB: " + ", ".join(f"{w} {g}: {d:.2e}" for (w, g), d in sorted(WORST.items())))
    assert WORST
