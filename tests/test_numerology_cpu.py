"""The checker of tests/test_gpu_numerology.py, checked without a GPU, and the host-side numerology of the library at every subcarrier spacing it accepts:

  * tests/_numerology_scenes.scene(30, ...) is conftest.make_scene byte for byte, and the table's scenes come out with the transform lengths, cyclic prefixes and target
    delays the table states (delays beyond the prefix at 60 / 120 kHz);
  * the host radarParams / cfar2D against the oracle, field for field, over 15 / 30 / 60 / 120 kHz x 11 / 24 / 66 / 135 / 273 PRB x numSlots default / 3 / 6;
  * the two independent restatements -- NumPy oracle and C++ port (oracle/cpu_port) -- on all eight scenes, with the assertions of test_cpu_port.py;
  * every scene and every antenna at least 1e-6 (relative) from a CA-CFAR threshold, and with a detection: the precondition of the exact list comparisons on the device,
    asserted here and there, never skipped;
  * csrc/ofdm_symbol.hpp through a small host program (tests/ofdm_symbol_host.cpp, built as test_beam_window_cpu.py builds its own) against oracle.cp_lengths /
    oracle.symbol_starts: numerology(), cp_of_symbol(), symbol_start() for Nfft 128 ... 4096, the four spacings, symbols 0 ... 2 sym_per_half + 1, and the whole-symbol count
    (isac_ofdm_symbol_count's rule) of a waveform that ends one sample before, on and one sample after the start of each of those symbols -- from the header and from the
    built library's own isac_ofdm_symbol_count / isac_ofdm_waveform_length."""
from __future__ import annotations

import ctypes
import os
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import oracle as O
from oracle import cpu_port as P
import _numerology_scenes as N
from conftest import ROOT, PKG_NAME, load_pkg, make_scene

CSRC = os.path.join(ROOT, PKG_NAME, "csrc")
SPACINGS = (15, 30, 60, 120)
NFFTS = (128, 256, 512, 1024, 2048, 4096)


# ---------------------------------------------------------------- the scene builder
@pytest.mark.parametrize("kw", [
    dict(n_ants=4, n_slots=4, nrb=24, targets=((150.0, 40.0, 1.5),), velocity=(0.0,), num_slots_param=6, zero_s_slots=False),
    dict(n_ants=6, n_slots=8, nrb=51, targets=((120.0, 60.0, 1.5), (-250.0, 80.0, 1.5)), velocity=(10.0, -6.0), num_slots_param=12, seed=5),
])
def test_scene_at_30_khz_is_make_scene(kw):
    want = make_scene(**kw)
    kw = dict(kw)
    got = N.scene(30, kw.pop("nrb"), kw.pop("n_ants"), kw.pop("n_slots"), kw.pop("targets"), kw.pop("velocity"), kw.pop("num_slots_param"), kw.pop("zero_s_slots", True), **kw)
    for f in ("tx_grid", "tx_wave", "noise"):
        g, w = getattr(got, f), getattr(want, f)
        assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes(order="F") == w.tobytes(order="F"), f
    assert sorted(vars(got.rp)) == sorted(vars(want.rp))
    for f, w in vars(want.rp).items():
        g = getattr(got.rp, f)
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), f
        elif f == "antennaType":
            assert vars(g) == vars(w)
        else:
            assert g == w and type(g) is type(w), f
    assert (got.K, got.L, got.A, got.T, got.amp) == (want.K, want.L, want.A, want.T, want.amp) and np.array_equal(got.los, want.los)
    assert vars(got.carrier) == vars(want.carrier) and vars(got.wave) == vars(want.wave)


def test_table_is_the_specified_one():
    assert [(c.scs, c.nrb, c.n_ants, c.n_slots, c.num_slots_param, len(c.targets), c.zero_s_slots) for c in N.CASES] == [
        (15, 24, 4, 4, 6, 1, False), (15, 52, 3, 4, 5, 2, True), (60, 24, 4, 4, 6, 1, False), (60, 66, 3, 8, 10, 2, True),
        (120, 24, 4, 8, 10, 1, False), (120, 66, 3, 8, 9, 2, True), (120, 11, 2, 4, 6, 1, False), (60, 11, 2, 4, 6, 1, False)]
    for c in N.CASES:
        sc = N.oracle_of(c).sc
        base, long_ = (int(v) for v in O.cp_lengths(sc.wave.Nfft, c.scs, 2)[::-1])
        assert (sc.wave.Nfft, sc.L, sc.rp.nFFT, (base, long_), N.delays_of(sc.rp)) == (c.nfft, c.L, c.n_fft, c.cp, c.delay), c.name
        assert sc.tx_grid.shape == (12 * c.nrb, c.L, c.n_ants)
    for scs in (15, 60, 120):                                              # each spacing has scenes that hold its numerology's second long-CP symbol (symbol 7 * 2^mu)
        assert sum(c.L > 7 * scs // 15 for c in N.CASES if c.scs == scs) >= 2
    # what the 30 kHz scenes hardly touch: a target later than the normal prefix, later than the long one, and two targets whose delays differ by more than it
    assert any(max(c.delay) > c.cp[0] for c in N.CASES if c.scs == 60) and sum(min(c.delay) > c.cp[0] for c in N.CASES if c.scs == 120) >= 2
    assert any(max(c.delay) > c.cp[1] for c in N.CASES) and any(max(c.delay) - min(c.delay) > c.cp[0] for c in N.CASES)
    for scs, edges in N.LONG_CP_EDGES.items():
        second = 7 * scs // 15                                                                     # index of the second long-CP symbol
        assert edges[:3] == (1, second, second + 1) and (len(edges) == 3 or edges[3] == 2 * second + 1)
        cps = O.cp_lengths(4096, scs, 2 * second + 1)
        assert [int(i) for i in np.flatnonzero(cps != cps[1])] == [0, second, 2 * second]


# ---------------------------------------------------------------- host parameter preparation
@pytest.mark.parametrize("scs", SPACINGS)
def test_host_radar_params_and_cfar_config_match_oracle_at_every_spacing(scs):
    pkg = load_pkg()
    n = 0
    for nrb in (11, 24, 66, 135, 273):
        for num_slots in (None, 3, 6):
            ci = SimpleNamespace(NRBsDL=nrb, SubcarrierSpacing=scs)
            wi = O.nr_ofdm_info(nrb, scs)
            cell = O.default_cell_params(n_ants=5, target_pos=N.PAIR, velocity=(10.0, -6.0))
            if num_slots is not None:
                cell.numSlots = num_slots
            got, want = pkg.sensing.radarParams(cell, ci, wi), O.radar_params(cell, ci, wi)
            lib_wi = pkg.sensing._marshal.nr_ofdm_info(nrb, scs)
            assert (lib_wi.Nfft, lib_wi.SampleRate, lib_wi.SymbolsPerSlot) == (wi.Nfft, wi.SampleRate, wi.SymbolsPerSlot)
            for f in ("fc", "fs", "Tsri", "N0", "nIFFT", "nFFT", "rRes", "vRes", "rMax", "vMax", "Pfa", "nTxAnts", "nTargets", "txPower"):
                assert getattr(got, f) == getattr(want, f), (f, nrb, num_slots)
            for f in ("range", "velocity", "largeScaleFading", "snrdB", "RxSteeringVec", "cfarEstZone"):
                assert np.array_equal(getattr(got, f), getattr(want, f)), (f, nrb, num_slots)
            cg, cw = pkg.sensing.detection.cfar2D(got), O.cfar2d_config(want)
            assert np.array_equal(cg.CUTIdx, cw.CUTIdx) and cg.CUTIdx.shape[1] >= 1
            assert cg.cfarDetector2D.GuardBandSize == cw.GuardBandSize == (2, 2) and cg.cfarDetector2D.TrainingBandSize == cw.TrainingBandSize == (1, 1)
            assert cg.cfarDetector2D.ProbabilityFalseAlarm == cw.Pfa == 1e-9
            n += 1
    assert n == 15


# ---------------------------------------------------------------- the two restatements on the table
@pytest.mark.parametrize("case", N.CASES, ids=lambda c: c.name)
def test_cpu_port_matches_oracle_on_the_table(case, record_property):
    o = N.oracle_of(case)
    sc = o.sc
    got_echo = P.mono_static_sensing(sc.tx_wave, sc.tx_grid.shape, sc.carrier, sc.rp, sc.los, sc.noise, nfft=sc.wave.Nfft)
    e_err = N.rel(got_echo, o.echo)
    record_property("echo_rel", e_err)
    assert got_echo.shape == o.echo.shape and e_err < 1e-10
    got, gdbg = P.fft2d(sc.rp, o.cfg, o.echo, sc.tx_grid, return_debug=True)
    r0, c0 = gdbg.first_row - 1, gdbg.first_col - 1
    nr, nc, _ = gdbg.power_window.shape
    assert N.rel(gdbg.power_window, np.abs(o.dbg.rdm[r0:r0 + nr, c0:c0 + nc, :]) ** 2) < 1e-10
    for a in range(sc.A):
        assert np.array_equal(gdbg.detections[a], o.dbg.detections[a]), f"antenna {a}"
    assert np.array_equal(got.rngEst, o.est.rngEst) and np.array_equal(got.velEst, o.est.velEst)
    assert np.array_equal(got.aziEst, o.est.aziEst) and got.rngEst.size >= 1
    assert N.rel(gdbg.Ra, o.dbg.Ra) < 1e-10 and np.array_equal(gdbg.Ra, gdbg.Ra.conj().T)


@pytest.mark.parametrize("case", N.CASES, ids=lambda c: c.name)
def test_table_scenes_are_far_from_a_threshold_and_detect(case, record_property):
    """The precondition of every exact list comparison on these scenes: asserted (the table says it holds with three or more orders to spare), never a reason to skip."""
    o = N.oracle_of(case)
    record_property("guard_margin", min(o.margin))
    print(f"{case.name}: guard margin {min(o.margin):.2e}, detections per antenna {[d.shape[1] for d in o.dbg.detections]}, rngEst {o.est.rngEst}")
    assert len(o.margin) == case.n_ants and all(m >= 1e-6 for m in o.margin), o.margin
    assert all(d.shape[1] >= 1 for d in o.dbg.detections) and o.est.rngEst.size >= 1


# ---------------------------------------------------------------- csrc/ofdm_symbol.hpp on the host
def run_host_program(tmp_path, include_dir=CSRC, flags=()):
    """Build tests/ofdm_symbol_host.cpp against the header in `include_dir` and return what it printed."""
    gxx = shutil.which("g++")
    assert gxx, "no host C++ compiler"
    exe = os.path.join(str(tmp_path), "ofdm_symbol_host")
    cmd = [gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", include_dir, os.path.join(ROOT, "tests", "ofdm_symbol_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def oracle_layout(nfft, scs, n_sym):
    """(starts [n_sym + 1], cps [n_sym + 1], ends [n_sym + 1]) from oracle.symbol_starts alone."""
    starts, cps = O.symbol_starts(nfft, scs, n_sym + 1)
    return starts, cps, starts + cps + nfft


def whole_symbols(ends, t):
    """Whole symbols in a waveform of t samples, as oracle.ofdm_demodulate counts them."""
    return int(np.searchsorted(ends, t, side="right"))


def compare_with_oracle(text, spacings=SPACINGS):
    """Every line the host program printed against the oracle; returns the number of values compared."""
    numerologies, symbols = {}, {}
    for line in text.splitlines():
        tag, *v = line.split()
        v = [int(x) for x in v]
        if tag == "N":
            numerologies[(v[0], v[1])] = tuple(v[2:])
        else:
            assert tag == "S"
            symbols[(v[0], v[1], v[2])] = tuple(v[3:])
    assert sorted(numerologies) == sorted((n, s) for n in NFFTS for s in SPACINGS)
    n = 0
    for nfft in NFFTS:
        for scs in spacings:
            mu = {15: 0, 30: 1, 60: 2, 120: 3}[scs]
            last = 2 * 7 * 2 ** mu + 1
            starts, cps, ends = oracle_layout(nfft, scs, last + 2)
            long_at = np.flatnonzero(cps != cps[1])
            assert numerologies[(nfft, scs)] == (mu, int(cps[1]), int(cps[0]), int(long_at[1])), (nfft, scs, numerologies[(nfft, scs)])
            for l in range(last + 1):
                s = int(starts[l])
                want = (int(cps[l]), s, whole_symbols(ends, s - 1), whole_symbols(ends, s), whole_symbols(ends, s + 1))
                assert symbols[(nfft, scs, l)] == want, (nfft, scs, l, symbols[(nfft, scs, l)], want)
                assert want[2:] == ((max(l - 1, 0), l, l))                   # the rule itself: a waveform that ends where symbol l starts holds l whole symbols
                n += 5
    assert len(symbols) == sum(len(NFFTS) * (2 * 7 * s // 15 + 2) for s in SPACINGS)
    return n


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan_ubsan"])
def test_ofdm_symbol_header_on_the_host(tmp_path, flags):
    n = compare_with_oracle(run_host_program(tmp_path, flags=flags))
    print(f"ofdm_symbol.hpp: {n} values equal to the oracle's")
    assert n == 5 * 6 * (16 + 30 + 58 + 114)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    p = load_pkg().library_path()
    assert os.path.exists(p)
    return ctypes.CDLL(p)


@pytest.mark.parametrize("scs", SPACINGS)
def test_library_symbol_count_and_waveform_length_at_every_spacing(lib, scs):
    """The built library's host entry points (csrc/echo.hip: geom_of, whole_symbols) on the same grid of lengths: they take the carrier's spacing, not a fixed one."""
    pkg = load_pkg()
    last = 2 * 7 * scs // 15 + 1
    for nfft in NFFTS:
        car = pkg._lib.Carrier(nfft // 2, nfft, scs, 0)
        starts, _, ends = oracle_layout(nfft, scs, last + 2)
        t, cnt = ctypes.c_int64(0), ctypes.c_int32(-1)
        for l in range(last + 1):
            assert lib.isac_ofdm_waveform_length(ctypes.byref(car), ctypes.c_int32(l), ctypes.byref(t)) == 0 and t.value == int(starts[l]), (nfft, l)
            for d in (-1, 0, 1):
                tt = int(starts[l]) + d
                if tt < 0:
                    continue
                assert lib.isac_ofdm_symbol_count(ctypes.byref(car), ctypes.c_int64(tt), ctypes.byref(cnt)) == 0
                assert cnt.value == whole_symbols(ends, tt), (nfft, l, d, cnt.value)


def test_lazy_cpi_case_at_120_khz_is_suitable():
    """tests/_lazy_cpi_reference.py with the spacing as an argument: the 120 kHz case of tests/test_gpu_numerology.py on the REFERENCE grid -- a decade inside both guards of
    tests/test_gpu_lazy_oracle.py, with detections, its last symbol behind the second long prefix, both targets later than the normal prefix and one later than the long one."""
    import _lazy_cpi_reference as R
    case = N.lazy_cpi_case_120()
    sc, e, _, _, eta = R.reference_of(case)
    assert case.scs == 120 and sc.wave.SampleRate == 4096 * 120e3 and sc.orp.nIFFT == 4096 and sc.orp.nFFT == 128 and (sc.K, sc.L_whole, sc.L_out, sc.A) == (1548, 57, 57, 49)
    assert sc.T == int(O.symbol_starts(4096, 120, 58)[0][57]) == 57 * (4096 + 288) + 2 * 256
    assert N.delays_of(sc.orp) == (348, 866)                               # the normal prefix is 288 samples, the long one 544
    o = R.oracle_chain(sc, e)
    print(f"{case.name}: detections {o.n_det}, CFAR margin {o.cfar_margin:.2e}, eigenvalue gap {o.eig_gap:.2e} w[0]")
    assert o.cfar_margin > 1e-6 and o.eig_gap > 1e-8 and o.n_det > 0 and o.est is not None
    assert eta < 1e-6 * float(np.abs(e).max())
    assert all(c.scs == 30 for c in tuple(R.TABLE) + tuple(R.NEIGHBOURS))      # the spacing argument defaults to the table's
