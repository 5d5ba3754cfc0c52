"""The tail of applyChannelModel without a GPU: the new ABI symbols, the host-side scalars (TR 38.901 path loss, fspl, thermal noise, DFT channel matrix) against
tests/_rx_frontend_restatement.py, self-checks that pin the transcription of Table 7.4.1-1 without MATLAB, and the code generation of the streaming kernel."""
from __future__ import annotations

import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest

import _rx_frontend_restatement as R
from conftest import ROOT, load_pkg

NEW_SYMBOLS = ("isac_path_loss_38901", "isac_path_loss_fspl", "isac_thermal_noise_power", "isac_dft_channel_matrix", "isac_rx_frontend_batch_dev", "isac_rx_frontend_dev")
D2D = (1.0, 10.0, 35.0, 100.0, 500.0, 2000.0, 5000.0)
H_UT = (1.5, 10.0)
H_BS = (10.0, 25.0, 35.0)
FC = (0.7e9, 3.5e9, 28e9)


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    return load_pkg()


@pytest.fixture(scope="module")
def PL(pkg):
    return pkg.communication.pathlossModels


def grid():
    for hu, hb, fc, d2 in itertools.product(H_UT, H_BS, FC, D2D):
        yield fc, (0.0, 0.0, hb), (d2, 0.0, hu)


def test_symbols_declared_exported_and_abi_still_8(pkg):
    hdr = open(os.path.join(ROOT, "include", "isac.h")).read()
    lib = C.CDLL(pkg.library_path())
    for s in NEW_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", hdr), s + " not declared in include/isac.h"
        assert hasattr(lib, s), s + " not exported"
        assert s in pkg._lib.HEADER_PROTOTYPES["isac.h"], s + " not in _lib.HEADER_PROTOTYPES"
    assert "isac_rx_frontend_job" in hdr and "isac_path_loss_config" in hdr
    assert lib.isac_abi_version() == 8 == pkg._lib.ISAC_ABI_VERSION and re.search(r"#define ISAC_ABI_VERSION 8\b", hdr)
    assert lib.isac_abi_sizeof(C.c_int32(9)) == C.sizeof(pkg._lib.RxFrontendJob) == 48
    assert lib.isac_abi_sizeof(C.c_int32(10)) == C.sizeof(pkg._lib.PathLossConfig) == 32


def test_path_loss_matches_the_restatement_on_the_grid(PL):
    """9 scenarios x LoS / NLoS x the grid: the same formulas in fp64 on both sides, |difference| <= 1e-12 dB (a few ulp of 200 dB)."""
    worst = 0.0
    n = 0
    for sc, los in itertools.product(R.SCENARIOS, (1, 0)):
        for fc, bs, ue in grid():
            got, want = PL.config5GNRModels(sc, fc, los, bs, ue), R.path_loss_38901(sc, fc, los, bs, ue)
            worst = max(worst, abs(got - want))
            assert abs(got - want) <= 1e-12, (sc, los, fc, bs, ue, got, want)
            n += 1
    assert n == 9 * 2 * 7 * 2 * 3 * 3
    print(f"path loss: {n} grid points, worst |C - restatement| = {worst:.3e} dB")


def test_nlos_is_never_below_los_and_inf_hh_ignores_los(PL):
    for sc in R.SCENARIOS:
        for fc, bs, ue in grid():
            a, b = PL.config5GNRModels(sc, fc, 1, bs, ue), PL.config5GNRModels(sc, fc, 0, bs, ue)
            assert b >= a, (sc, fc, bs, ue, a, b)
            if sc == "InF-HH":
                assert a == b
    assert any(PL.config5GNRModels("InF-SH", fc, 0, bs, ue) > PL.config5GNRModels("InF-SH", fc, 1, bs, ue) for fc, bs, ue in grid())


@pytest.mark.parametrize("scenario", ["UMa", "UMi", "RMa"])
def test_los_branches_meet_at_the_breakpoint(PL, scenario):
    """|PL1 - PL2| <= 1e-9 dB at d2D = d'BP: through the library (d2D = d'BP takes the first branch, the next double above it the second) and on the restated
    branch formulas.  UMa / UMi: for every height pair of the grid (PL2's -9 log10(d'BP^2 + dh^2) equals -18 log10 d3D there, so 40 - 18 = 22 -- a wrong
    coefficient in either branch shows).  RMa: the table anchors PL2 at PL1(d_BP) with d3D = d_BP, so the two branches meet where d3D = d2D, i.e. for
    equal heights (with unequal heights the table itself steps by 40 log10(d3D / d_BP) - (PL1(d3D) - PL1(d_BP)), ~1e-4 dB at d_BP ~ 4 km);
    the library is checked at the equal-height point of the grid (10 m, 10 m), the restated branches at d = d_BP for every height pair."""
    n = 0
    for hu, hb, fc in itertools.product(H_UT, H_BS, FC):
        if scenario == "RMa":
            dbp = R.breakpoint_rma(fc, hb, hu)
            p1, p2 = R.rma_los_branches(dbp, fc / 1e9, dbp, 5.0)
            assert abs(p1 - p2) <= 1e-9
            if hu != hb:
                continue
        else:
            dbp = R.breakpoint_uma_umi(fc, hb, hu)
            d3 = math.sqrt(dbp ** 2 + (hb - hu) ** 2)
            p1, p2 = (R.uma_los_branches if scenario == "UMa" else R.umi_los_branches)(d3, fc / 1e9, dbp, hb, hu)
            assert abs(p1 - p2) <= 1e-9
        assert dbp > 0
        at = PL.config5GNRModels(scenario, fc, 1, (0.0, 0.0, hb), (dbp, 0.0, hu))
        above = PL.config5GNRModels(scenario, fc, 1, (0.0, 0.0, hb), (math.nextafter(dbp, math.inf), 0.0, hu))
        far = PL.config5GNRModels(scenario, fc, 1, (0.0, 0.0, hb), (4.0 * dbp, 0.0, hu))
        near = PL.config5GNRModels(scenario, fc, 1, (0.0, 0.0, hb), (dbp / 4.0, 0.0, hu))
        assert abs(at - above) <= 1e-9, (hu, hb, fc, at, above)
        if scenario != "RMa":                                                                            # (RMa's PL1 carries a term linear in d: no clean slopes)
            assert (far - at) > 1.5 * (at - near) > 0, "the slope must steepen beyond the breakpoint"   # 40 dB / decade against 21-22
        n += 1
    assert n == (3 if scenario == "RMa" else 18)


def test_equal_positions_and_fspl(PL):
    for sc in R.SCENARIOS:
        assert PL.config5GNRModels(sc, 3.5e9, 1, (3.0, 4.0, 5.0), (3.0, 4.0, 5.0)) == 0.0
        assert PL.config5GNRModels(sc, 3.5e9, 0, (3.0, 4.0, 5.0), (3.0, 4.0, 5.0)) == 0.0
    fc = 3.5e9
    lam = R.C0 / fc
    assert PL.configFreeSpaceModel(fc, (1.0, 2.0, 3.0), (1.0, 2.0, 3.0)) == 0.0                          # R = 0
    assert PL.configFreeSpaceModel(fc, (0.0, 0.0, 0.0), (0.5 * lam / (4 * math.pi), 0.0, 0.0)) == 0.0      # R < lambda / 4 pi
    for r in (0.01, 1.0, 35.0, 2000.0):
        bs, ue = (1.0, -2.0, 25.0), (1.0 + r * 0.6, -2.0 + r * 0.8, 25.0)
        want = 20.0 * math.log10(4.0 * math.pi * math.dist(bs, ue) * fc / R.C0)
        got = PL.configFreeSpaceModel(fc, bs, ue)
        assert abs(got - want) <= 1e-12 and abs(got - R.fspl(fc, bs, ue)) <= 1e-12
        assert PL.configFreeSpaceModel(fc, ue, bs) == got                                                  # symmetric in the two positions
    # ... and the TR 38.901 model is NOT: h_BS is the first position's height (the downlink call of the reference passes the UE first, uePhy.m:744)
    gnb, ue = (0.0, 0.0, 25.0), (100.0, 0.0, 1.5)
    a, b = PL.config5GNRModels("UMa", fc, 0, gnb, ue), PL.config5GNRModels("UMa", fc, 0, ue, gnb)
    assert abs(a - b) > 1.0, (a, b)
    assert abs(a - R.path_loss_38901("UMa", fc, 0, gnb, ue)) <= 1e-12 and abs(b - R.path_loss_38901("UMa", fc, 0, ue, gnb)) <= 1e-12


def test_optional_models_and_config_fields(PL):
    bs, ue, fc = (0.0, 0.0, 25.0), (300.0, 0.0, 1.5), 3.5e9
    d = math.dist(bs, ue)
    for sc, slope in (("UMa", 30.0), ("UMi", 31.9), ("InH", 31.9)):
        assert abs(PL.config5GNRModels(sc, fc, 0, bs, ue, OptionalModel=True) - (32.4 + 20.0 * math.log10(3.5) + slope * math.log10(d))) <= 1e-12
        assert PL.config5GNRModels(sc, fc, 1, bs, ue, OptionalModel=True) == PL.config5GNRModels(sc, fc, 1, bs, ue)
    assert abs(PL.config5GNRModels("RMa", fc, 0, bs, ue, BuildingHeight=8.0, StreetWidth=30.0) - R.path_loss_38901("RMa", fc, 0, bs, ue, h=8.0, w=30.0)) <= 1e-12
    assert abs(PL.config5GNRModels("UMa", fc, 1, bs, (5000.0, 0.0, 1.5), EnvironmentHeight=1.2) - R.path_loss_38901("UMa", fc, 1, bs, (5000.0, 0.0, 1.5), he=1.2)) <= 1e-12
    with pytest.raises(ValueError):
        PL.config5GNRModels("UMx", fc, 1, bs, ue)


def test_thermal_noise_power(pkg):
    f = pkg.communication.phyLayer.thermalNoisePower
    for fs in (15.36e6, 122.88e6):
        assert f(290.0, 0.0, fs) == R.KB * 290.0 * fs
    for t, nf, fs in ((290.0, 7.0, 122.88e6), (300.0, 5.0, 61.44e6), (150.0, 2.5, 15.36e6)):
        got, want = f(t, nf, fs), R.thermal_noise_power(t, nf, fs)
        assert abs(got - want) <= math.ulp(want), (t, nf, fs, got, want)


@pytest.mark.parametrize("nt,nr", [(64, 2), (2, 64), (4, 4), (1, 1)])
def test_dft_channel_matrix(pkg, nt, nr):
    h = pkg.communication.phyLayer.dftChannelMatrix(nt, nr)
    n = max(nt, nr)
    assert h.shape == (nt, nr)
    assert np.abs(h - np.fft.fft(np.eye(n))[:nt, :nr] / np.sqrt(n)).max() <= 1e-15
    assert np.abs(h - R.dft_channel_matrix(nt, nr)).max() <= 1e-15
    assert abs(np.linalg.norm(h, 2) - 1.0) <= 1e-14


# ---------------------------------------------------------------- code generation of the streaming kernel (as tests/test_isa_cpu.py checks the other hot kernels)
LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, "llvm-objdump")), reason="ROCm LLVM tools not installed")
def test_front_end_kernel_code_generation(pkg, tmp_path):
    from test_isa_cpu import CodeObject
    co = CodeObject(str(tmp_path), "rxfe")
    for mode, loads in ((0, 2), (1, 4), (2, 2)):                                   # none / injected / Philox: elements in flight per thread x arrays read
        name, meta, asm = co.find("rxfe_kernel", f"ILi{mode}E")
        assert meta["private_segment_fixed_size"] == 0, meta                        # no scratch
        assert meta["vgpr_count"] <= 64 and meta["agpr_count"] == 0, meta           # eight waves per SIMD
        assert meta.get("group_segment_fixed_size", 0) == 0, meta                   # no LDS
        assert sum(ln.startswith("global_load_dwordx4") for ln in asm) == loads, name
        assert sum(ln.startswith("global_store_dwordx4") for ln in asm) == 2, name
        assert not any(ln.startswith(("flat_", "scratch_", "global_load_dword ", "global_load_dwordx2", "global_store_dword ", "global_store_dwordx2")) for ln in asm), name
