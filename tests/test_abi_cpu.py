"""CPU-side checks of the drop-in boundary: the library builds for gfx950 without a GPU,
loads, exports every symbol include/isac.h declares, and the host-side mirrors of the
reference functions (radarParams, cfar2D, updateCDLModels) agree with the oracle."""
from __future__ import annotations

import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import _abi_header as H
import oracle as O
from conftest import load_pkg, make_scene


@pytest.fixture(scope="module")
def lib_path():
    import __graft_entry__ as g
    g.build()
    p = load_pkg().library_path()
    assert os.path.exists(p)
    return p


def test_header_symbols_all_exported(lib_path):
    hdr = H.text("isac.h")
    declared = set(re.findall(r"\b(isac_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"isac_status"}
    lib = ctypes.CDLL(lib_path)
    missing = [s for s in sorted(declared) if not hasattr(lib, s)]
    assert not missing, f"declared in isac.h but not exported: {missing}"
    pkg = load_pkg()
    assert set(pkg._lib.HEADER_PROTOTYPES["isac.h"]) == declared
    m = re.search(r"#define ISAC_ABI_VERSION (\d+)", hdr)
    assert lib.isac_abi_version() == int(m.group(1)) == pkg._lib.ISAC_ABI_VERSION >= 3
    # struct sizes as the library was built == the ctypes mirrors (the loader refuses a mismatch): every ISAC_SIZEOF_* of every header, enum or #define
    L = pkg._lib
    selectors = H.sizeof_selectors()
    assert sorted(selectors) == list(range(13)) and sorted(i for i, (header, _) in selectors.items() if header == "isac.h") == list(range(11))
    assert len(re.findall(r"\bISAC_SIZEOF_\w+ = \d+", H.without_comments("isac.h"))) == 11                           # ... those eleven in the enum form
    assert selectors[11] == ("isac_targets.h", "TARGET_LIST") and selectors[12] == ("isac_cfar.h", "CFAR_METHOD")
    assert [name for name, _ in L.ABI_STRUCTS] == ["isac_" + selectors[i][1].lower() for i in range(13)]
    for which, (name, cls) in enumerate(L.ABI_STRUCTS):
        assert lib.isac_abi_sizeof(ctypes.c_int32(which)) == ctypes.sizeof(cls), name
    assert lib.isac_abi_sizeof(ctypes.c_int32(13)) == -1
    assert lib.isac_abi_sizeof(ctypes.c_int32(99)) == -1


# ---- the prototype table of _lib.py against the headers, by the parser and the typing rule of tests/_abi_header.py.  One row per header: its functions in the
#      header's order, each with its argument count; None = isac.h proper, whose 77 names come from the header.  A new entry point adds one row (or one pair) here.
HEADERS = {
    "isac.h": None,
    "isac_targets.h": [("isac_fft2d_get_targets", 4)],
    "isac_cfar.h": [("isac_cfar_threshold_factor", 5), ("isac_cfar2d", 13), ("isac_fft2d_redetect", 8)],
    "isac_cfar_mc.h": [("isac_cfar_monte_carlo", 11)],
    "isac_lazy_cov.h": [("isac_ctx_set_lazy_cov_route", 2), ("isac_ctx_get_lazy_cov_route_used", 2)],
    "isac_targets_upa.h": [("isac_fft2d_get_targets_upa", 5)],
    "isac_beams.h": [("isac_fft2d_get_rdm_window", 6), ("isac_fft2d_beam_detect", 13)],
    "isac_refine.h": [("isac_fft2d_refine_targets", 17)],
    "isac_clean.h": [("isac_fft2d_clean_targets", 23)],
    "isac_relax.h": [("isac_fft2d_relax_targets", 18)],
    "isac_directions.h": [("isac_resolve_directions", 19)],
    "isac_beam_clean.h": [("isac_fft2d_beam_clean_targets", 30)],
    "isac_multistatic.h": [("isac_multi_static_channel_dev", 20), ("isac_multi_static_sensing_dev", 23)],
    "isac_cancel_paths.h": [("isac_cancel_paths_dev", 19)],
}


@pytest.mark.parametrize("header", list(HEADERS))
def test_prototype_table_matches_the_header(lib_path, header):
    L = load_pkg()._lib
    protos = H.prototypes(header)
    table = L.HEADER_PROTOTYPES[header]
    if header == "isac.h":
        assert len(protos) == 77 == len(set(re.findall(r"\b(isac_[a-z0-9_]+)\s*\(", H.text(header))) - {"isac_status"})   # the regex found every declaration
        counts = {name: len(types) for _, name, types in protos}
        # once, over all headers: the keys are isac.h and its #include lines in order, and no name stands under two headers
        assert list(L.HEADER_PROTOTYPES) == ["isac.h"] + H.includes() == list(HEADERS)
        assert sum(len(t) for t in L.HEADER_PROTOTYPES.values()) == len(L.PROTOTYPES) == 95 and len(table) == 77
    else:
        assert header in H.includes()                                                                                 # isac.h includes it
        assert [name for _, name, _ in protos] == [name for name, _ in HEADERS[header]]
        counts = dict(HEADERS[header])
    assert [name for _, name, _ in protos] == list(table)                                                             # same names, in the header's order
    for ret, name, types in protos:
        restype, argtypes = table[name]
        assert restype is H.RETURNS[ret], name
        assert len(argtypes) == len(types) == counts[name], name
        for i, (got, c_type) in enumerate(zip(argtypes, types)):
            assert got is H.rule(c_type, L), f"{name} argument {i}: {c_type}"
    lib = L.load()
    for name, (restype, argtypes) in table.items():                                                                  # and load() applied the table
        fn = getattr(lib, name)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name


def test_option_and_status_constants_match_the_header():
    L = load_pkg()._lib
    hdr = H.without_comments("isac.h")
    opts = {n: int(v) for n, v in re.findall(r"\bISAC_OPT_(\w+) = (\d+)", hdr)}
    assert len(opts) == 5 and opts == {n[4:]: getattr(L, n) for n in dir(L) if n.startswith("OPT_")}
    body = re.search(r"typedef enum \{([^}]*)\} isac_status;", hdr).group(1)
    status = {int(v): n for n, v in re.findall(r"\bISAC_(?:ERR_)?(\w+) = (\d+)", body)}
    assert len(status) == 9 and status == L.STATUS_NAMES


def test_prototypes_reject_a_wrong_call_and_pass_64_bit_values(lib_path):
    """Through load(), with plain Python arguments.  A float for int64_t T is a ctypes.ArgumentError; one argument too few is refused by
    ctypes before the call as well, as a TypeError ("this function takes at least 3 arguments": ctypes raises ArgumentError for a
    conversion only).  T = 2**33 reaches the library whole: the symbol count n it returns brackets T."""
    L = load_pkg()._lib
    lib = L.load()
    car = L.Carrier(3276, 4096, 30, 0)
    n = ctypes.c_int32(0)
    with pytest.raises(ctypes.ArgumentError):
        lib.isac_ofdm_symbol_count(ctypes.byref(car), 983040.0, ctypes.byref(n))
    with pytest.raises(TypeError, match="at least 3 arguments"):
        lib.isac_ofdm_symbol_count(ctypes.byref(car), 983040)
    T = 2 ** 33
    assert lib.isac_ofdm_symbol_count(ctypes.byref(car), T, ctypes.byref(n)) == 0
    lo, hi = ctypes.c_int64(0), ctypes.c_int64(0)
    assert lib.isac_ofdm_waveform_length(ctypes.byref(car), n.value, ctypes.byref(lo)) == 0
    assert lib.isac_ofdm_waveform_length(ctypes.byref(car), n.value + 1, ctypes.byref(hi)) == 0
    print(f"T = {T}: n = {n.value}, waveform_length(n) = {lo.value}, waveform_length(n + 1) = {hi.value}")
    assert lo.value <= T < hi.value


def test_size_queries_need_no_gpu(lib_path):
    pkg = load_pkg()
    lib = pkg._lib.load()
    car = pkg._lib.Carrier(3276, 4096, 30, 0)
    n = ctypes.c_int32(0)
    assert lib.isac_ofdm_symbol_count(ctypes.byref(car), ctypes.c_int64(983040), ctypes.byref(n)) == 0 and n.value == 224
    assert lib.isac_ofdm_symbol_count(ctypes.byref(car), ctypes.c_int64(983039), ctypes.byref(n)) == 0 and n.value == 223
    t = ctypes.c_int64(0)
    assert lib.isac_ofdm_waveform_length(ctypes.byref(car), ctypes.c_int32(224), ctypes.byref(t)) == 0 and t.value == 983040
    car2 = pkg._lib.Carrier(288, 512, 30, 0)
    assert lib.isac_ofdm_waveform_length(ctypes.byref(car2), ctypes.c_int32(14), ctypes.byref(t)) == 0 and t.value == 7680
    starts, cps = O.symbol_starts(512, 30, 29)
    for l in (1, 13, 14, 15, 28):
        assert lib.isac_ofdm_waveform_length(ctypes.byref(car2), ctypes.c_int32(l), ctypes.byref(t)) == 0
        assert t.value == starts[l]


def test_product_fails_loudly_without_gpu(lib_path):
    pkg = load_pkg()
    if os.path.exists("/dev/kfd"):
        pytest.skip("GPU present")
    with pytest.raises(pkg.IsacError):
        pkg.Context()


def test_host_radar_params_and_cfar_config_match_oracle():
    pkg = load_pkg()
    for n_ants, targets, vel in [(16, ((100.0, 20.0, 1.5),), (7.0,)), (64, ((60.0, -40.0, 1.5), (-200.0, 100.0, 10.0)), (-3.0, 9.0))]:
        sc = make_scene(n_ants=n_ants, n_slots=1, nrb=24, targets=targets, velocity=vel, with_noise=False)
        got = pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)
        want = sc.rp
        for f in ("fc", "fs", "Tsri", "N0", "nIFFT", "nFFT", "rRes", "vRes", "rMax", "vMax", "Pfa"):
            assert getattr(got, f) == getattr(want, f), f
        for f in ("range", "velocity", "largeScaleFading", "snrdB", "RxSteeringVec", "cfarEstZone"):
            assert np.array_equal(getattr(got, f), getattr(want, f)), f
        cg, cw = pkg.sensing.detection.cfar2D(got), O.cfar2d_config(want)
        assert np.array_equal(cg.CUTIdx, cw.CUTIdx)
        assert cg.cfarDetector2D.GuardBandSize == (2, 2) and cg.cfarDetector2D.TrainingBandSize == (1, 1)
        assert cg.cfarDetector2D.ProbabilityFalseAlarm == 1e-9


def test_update_cdl_models():
    pkg = load_pkg()
    out = pkg.communication.channelModels.updateCDLModels(SimpleNamespace(numUEs=3, ueLoSConditions=[1, 0, 1]))
    assert out == ["CDL-D", "CDL-A", "CDL-D"]      # updateCDLModels.m:9-14


def test_cut_rectangle_recovery():
    pkg = load_pkg()
    from importlib import import_module
    f = import_module(pkg.__name__ + ".sensing.estimation.fft2D")
    sc = make_scene(n_ants=2, n_slots=1, nrb=24, with_noise=False)
    cf = pkg.sensing.detection.cfar2D(sc.rp)
    r0, r1, c0, c1 = f._cut_rectangle(cf.CUTIdx)
    assert (r0, r1) == (cf.CUTIdx[0, 0], cf.CUTIdx[0, -1]) and (c0, c1) == (cf.CUTIdx[1, 0], cf.CUTIdx[1, -1])
    with pytest.raises(pkg.IsacError):
        f._cut_rectangle(cf.CUTIdx[:, ::-1])


def test_mex_gateway_compiles_against_the_header():
    """The reference-side binding (mex/isac_mex.cpp) type-checks against include/isac.h."""
    import shutil
    import sys
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import __graft_entry__ as g
    g.check_mex_gateway()


def test_mex_gateway_links_against_the_test_runtime():
    """tests/_build/mex_host = the gateway + the in-process mx runtime + libisac_hip.so: it must link here (no GPU needed for that);
    without arguments it prints its usage and exits 1 before touching the device."""
    import subprocess
    import __graft_entry__ as g
    exe = g.build_mex_host()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "usage" in r.stderr
