"""Sub-sample range without a GPU (include/isac_subsample.h): the restatement of tests/_subsample_restatement.py against itself and the physics, the
conditioning of the scenes tests/test_gpu_subsample.py compares the device on, and the binding's lines for the stand-alone header.
  1. the ramp (a) equals the physical reference (b) to 1e-10 where d + delta <= CP / 2 - 1 and the paths have no Doppler shift; with one, they differ by the leakage bound
  2. the restated estimator recovers a noiseless tone to 1e-9 bin at the four shapes of the GPU test
  3. conditioning: |P'| at rho_ref +- 1e-6 is above 1e3 rounding bounds of the fp64 sums on every entry of every GPU scene, and no comparison of the peak rule is close
  4. the restated end-to-end chain stays within 0.05 bin of the truth
  5. the two lines of _lib.STANDALONE_PROTOTYPES re-derived from the header; the library exports both names"""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

import _abi_header as H
import _subsample_restatement as S
from conftest import load_pkg
from oracle.matlab_compat import kaiser

RTOL = 1e-10
E2E_BOUND = 0.05                                                            # bins; tests/test_gpu_subsample.py holds the device chain to twice this


# ---------------------------------------------------------------- 1
def test_ramp_equals_the_physically_delayed_signal():
    s = S.frac_scene("still")
    assert (s.paths.doppler == 0).all() and (s.paths.frac > 0).all() and len(set(s.paths.source.tolist())) == 2
    assert float((s.paths.shift + s.paths.frac).max()) <= s.cp / 2 - 1 and float((s.paths.shift + s.paths.frac).max()) > s.cp / 2 - 1.5   # up to the limit
    phys = S.frac_physical("still")
    err = float(np.abs(s.ramp - phys).max() / np.abs(phys).max())
    whole = S.frac_echo_ramp(s.waves, s.K, s.nfft, s.scs, s.rp.fc, s.rp.fs, s.A, s.rows, np.zeros(3))
    moved = float(np.abs(s.ramp - whole).max() / np.abs(phys).max())
    print(f"still: (a) against (b) {err:.3e} of max|grid|; the fractions move the grid by {moved:.3e} of it")
    assert moved > 0.1                                                      # the fractions are really there
    assert err <= RTOL


def test_ramp_with_a_doppler_shift_differs_by_the_leakage_only():
    """Not part of the definition's claim: with a Doppler shift (a) and (b) part at the size of the inter-carrier leakage times the ramp's slope; measured 9.1e-3 of
    max|grid| on this scene (-3.1 and +2.5 kHz at 60 kHz spacing), bound 7.4e-2 (tests/_subsample_restatement.py: ramp_leak_bound, six rms of the leaked sum)."""
    s = S.frac_scene("moving")
    phys = S.frac_physical("moving")
    keep = [p for p in range(3) if s.paths.shift[p] + s.paths.frac[p] <= s.cp / 2 - 1]      # (b) is the circular form only inside the limit
    rows, frac = [s.rows[p] for p in keep], s.paths.frac[keep]
    a = S.frac_echo_ramp(s.waves, s.K, s.nfft, s.scs, s.rp.fc, s.rp.fs, s.A, rows, frac)
    b = S.frac_echo_physical(s.grids, s.amps, s.K, s.nfft, s.scs, s.rp.fc, s.rp.fs, s.A, rows, frac, s.T)
    err = float(np.abs(a - b).max() / np.abs(b).max())
    bound = max(S.ramp_leak_bound(s.K, s.nfft, s.scs, r[2], d) for r, d in zip(rows, frac))
    print(f"moving: (a) against (b) {err:.3e} of max|grid|, leakage bound {bound:.3e}")
    assert len(keep) == 2 and RTOL < err <= bound


# ---------------------------------------------------------------- 2
@pytest.mark.parametrize("name", list(S.SHAPES))
def test_estimator_recovers_a_noiseless_tone(name):
    K, n_ifft, Ls, A, _ = S.SHAPES[name]
    rho, nu = 0.3 * n_ifft + 0.37, 0.123
    rx, tx = S.single_tone(K, n_ifft, Ls, A, rho, nu)
    r = S.range_refine(rx, tx, n_ifft, 64, [int(round(rho)) + 1], [nu])
    err = abs(r.rho[0] - rho)
    print(f"{name}: rho {r.rho[0]!r} for {rho!r}: {err:.3e} bin; power {r.power[0]:.6e}")
    assert r.status[0] == 0 and err <= 1e-9
    w = kaiser(K, 3.0)
    assert abs(r.power[0] / (A * (Ls * w.sum()) ** 2 / (n_ifft * 64.0)) - 1) < 1e-9      # the tone's coherent gain


# ---------------------------------------------------------------- 3
@pytest.mark.parametrize("name", list(S.SHAPES))
def test_gpu_scenes_are_conditioned(name):
    s = S.tone_scene(name)
    w = kaiser(s.K, 3.0)
    bound = S.dp_rounding_bound(s.rx, s.tx, s.n_ifft, s.n_fft)
    worst_dp, worst_gap = np.inf, np.inf
    for i in range(s.n):
        has_peak, gap = S.probe_margins(s.ref.c[i], w, s.n_ifft, s.n_fft, int(s.row[i]))
        worst_gap = min(worst_gap, gap)
        assert has_peak == (s.ref.status[i] == 0)
        if has_peak:
            lo, hi = (float(S.dp_ld(s.ref.c[i], w, s.n_ifft, s.n_fft, s.ref.rho[i] + d)) for d in (-1e-6, 1e-6))
            assert lo > 0 > hi                                              # a maximum
            worst_dp = min(worst_dp, lo / bound, -hi / bound)
    print(f"{name}: status {s.ref.status.tolist()}; |P'| at rho_ref +- 1e-6 >= {worst_dp:.3e} rounding bounds; closest comparison of the peak rule {worst_gap:.3e}")
    assert (s.ref.status == 1).sum() == (0 if name == "k288_a2" else 1) and s.ref.status[-1] == (0 if name == "k288_a2" else 1)
    assert worst_dp > 1e3 and worst_gap > 1e-6
    near = [abs(s.ref.rho[i] - t[0]) for i in range(s.n) if s.ref.status[i] == 0 for t in s.tones if abs(s.nu[i] - t[1]) < 0.01 and abs(s.ref.rho[i] - t[0]) < 1]
    assert len(near) == (s.ref.status == 0).sum() and max(near) < 0.05      # every entry found its tone off the bin


# ---------------------------------------------------------------- 4
def test_restated_end_to_end_chain():
    """Measured: errors 3.3e-4 and 1.9e-2 bin (the weaker, farther target; at the grid column's nu0, not a refined nu); the grid rows are 0.37 and 0.39 bin off.  With the
    two targets at nearly one Doppler (6 and -9 m/s) the farther one was off by 3.6e-2 bin: mutual bias, which the call leaves to a RELAX over range (out of scope)."""
    rho, truth, row = S.e2e_restated_chain()
    err, grid_err = np.abs(rho - truth), np.abs((row - 1) - truth)
    print(f"end to end, restated: rho {rho.tolist()} for {truth.tolist()}: errors {err.tolist()} bin; grid rows {row.tolist()} are {grid_err.tolist()} bin off")
    assert (err <= E2E_BOUND).all() and (grid_err > 0.3).all()


# ---------------------------------------------------------------- 5
@pytest.fixture(scope="module")
def lib_path():
    import __graft_entry__ as g
    g.build()
    p = load_pkg().library_path()
    assert os.path.exists(p)
    return p


def test_standalone_prototypes_match_the_header(lib_path):
    L = load_pkg()._lib
    header = "isac_subsample.h"
    assert list(L.STANDALONE_PROTOTYPES) == [header] and header not in H.includes() and header not in L.HEADER_PROTOTYPES
    assert re.search(r'^#include "isac\.h"', H.text(header), flags=re.M)
    protos = H.prototypes(header)
    table = L.STANDALONE_PROTOTYPES[header]
    assert [(name, len(types)) for _, name, types in protos] == [("isac_multi_static_sensing_frac_dev", 24), ("isac_range_refine_dev", 16)]
    assert [name for _, name, _ in protos] == list(table) and not set(table) & set(L.PROTOTYPES)
    for ret, name, types in protos:
        restype, argtypes = table[name]
        assert restype is H.RETURNS[ret], name
        assert len(argtypes) == len(types), name
        for i, (got, c_type) in enumerate(zip(argtypes, types)):
            assert got is H.rule(c_type, L), f"{name} argument {i}: {c_type}"
    # the frac call = isac_multi_static_sensing_dev's types with one pointer behind path_shift
    base = {name: types for _, name, types in H.prototypes("isac_multistatic.h")}["isac_multi_static_sensing_dev"]
    frac = protos[0][2]
    assert frac[:12] == base[:12] and frac[12] == "const double*" and frac[13:] == base[12:]
    raw = ctypes.CDLL(lib_path)
    assert all(hasattr(raw, name) for name in table)
    lib = L.load()
    for name, (restype, argtypes) in table.items():                         # and load() applied the table
        fn = getattr(lib, name)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name
    m = re.search(r"#define ISAC_ABI_VERSION (\d+)", H.text("isac.h"))
    assert int(m.group(1)) == 8 == L.ISAC_ABI_VERSION


def test_refusals_need_no_gpu(lib_path):
    """The NULL-context refusal of both calls, through the prototypes load() applied."""
    pkg = load_pkg()
    lib = pkg._lib.load()
    assert lib.isac_range_refine_dev(None, None, None, None, 1, 1, 1, None, None, 0, 0, None, None, None, None, None) == 1
    assert lib.isac_multi_static_sensing_frac_dev(*([None] * 3), 1, 1, 1.0, 1.0, 0.0, 1, 1, *([None] * 7), 0, None, 0, 1, None, None, None) == 1


def test_multi_static_paths_sub_sample_record():
    import _multistatic_restatement as M
    pkg = load_pkg()
    b = M.base()
    sc = b.sc
    kw = dict(carrierInfo=sc.carrier, waveInfo=sc.wave, directLoS=[1, 1])
    old = pkg.sensing.channelModels.multiStaticPaths(sc.cell, [sc.cell, b.nb.cell], b.targets, **kw)
    off = pkg.sensing.channelModels.multiStaticPaths(sc.cell, [sc.cell, b.nb.cell], b.targets, subSample=False, **kw)
    new = pkg.sensing.channelModels.multiStaticPaths(sc.cell, [sc.cell, b.nb.cell], b.targets, subSample=True, **kw)
    assert not hasattr(old, "frac") and not hasattr(off, "frac") and sorted(vars(off)) == sorted(vars(old))
    for f in ("source", "shift", "doppler", "gain", "rxSteering"):
        assert np.array_equal(getattr(old, f), getattr(off, f)) and getattr(old, f).dtype == getattr(off, f).dtype, f
    assert [r.tolist() for r in old.shift.reshape(-1, 1)] == [[int(v)] for v in [r[1] for r in M.restated_paths("interference")]]   # the reference's ceil, as before
    with pytest.raises(ValueError):                                         # the whole-sample calls refuse the record instead of taking its floor shifts
        pkg.sensing.channelModels.referencePaths(new)
    with pytest.raises(ValueError):
        pkg.sensing.cancelPaths(np.zeros((8, sc.A), dtype=np.complex128), [np.zeros((8, sc.A), dtype=np.complex128), None], sc.rp, new)
    with pytest.raises(ValueError):
        pkg.sensing.channelModels.multiStaticChannel([np.zeros((8, sc.A), dtype=np.complex128), None], sc.rp, new)
    old.frac = np.zeros(old.shift.size)                                     # all zero: the reference's model, taken
    assert len(pkg.sensing.channelModels.referencePaths(old).source) == len(pkg.sensing.channelModels.referencePaths(off).source) == 1
    assert new.frac.shape == new.shift.shape and ((new.frac >= 0) & (new.frac < 1)).all() and (new.frac > 0).all()
    assert np.array_equal(new.shift + (new.frac > 0), old.shift) and np.array_equal(new.gain, old.gain) and np.array_equal(new.doppler, old.doppler)
    delay_own = 2.0 * np.asarray(sc.rp.range) / 299792458.0 * sc.rp.fs
    own = [i for i, k in enumerate(new.kind) if k[0] == "target" and k[1] == 0]
    assert np.allclose(new.shift[own] + new.frac[own], delay_own, rtol=0, atol=1e-9)
