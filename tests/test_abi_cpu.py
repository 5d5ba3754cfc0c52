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

import oracle as O
from conftest import ROOT, load_pkg, make_scene


@pytest.fixture(scope="module")
def lib_path():
    import __graft_entry__ as g
    g.build()
    p = load_pkg().library_path()
    assert os.path.exists(p)
    return p


def test_header_symbols_all_exported(lib_path):
    hdr = open(os.path.join(ROOT, "include", "isac.h")).read()
    declared = set(re.findall(r"\b(isac_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"isac_status"}
    lib = ctypes.CDLL(lib_path)
    missing = [s for s in sorted(declared) if not hasattr(lib, s)]
    assert not missing, f"declared in isac.h but not exported: {missing}"
    pkg = load_pkg()
    assert set(pkg._lib.EXPORTS) == declared
    m = re.search(r"#define ISAC_ABI_VERSION (\d+)", hdr)
    assert lib.isac_abi_version() == int(m.group(1)) == pkg._lib.ISAC_ABI_VERSION >= 3
    # struct sizes as the library was built == the ctypes mirrors (the loader refuses a mismatch)
    L = pkg._lib
    selectors = {int(v): n for n, v in re.findall(r"\bISAC_SIZEOF_(\w+) = (\d+)", hdr)}
    assert [name for name, _ in L.ABI_STRUCTS] == ["isac_" + selectors[i].lower() for i in range(len(selectors))] and len(selectors) == 11
    for which, (name, cls) in enumerate(L.ABI_STRUCTS):
        assert lib.isac_abi_sizeof(ctypes.c_int32(which)) == ctypes.sizeof(cls), name
    assert lib.isac_abi_sizeof(ctypes.c_int32(99)) == -1


# ---- the prototype table of _lib.py against include/isac.h.  The typing rule is restated here, not imported from the binding:
#      by-value scalars by their C type, a pointer to a struct the binding mirrors -> POINTER(mirror), every other pointer (T[] parameters included) -> c_void_p.
_SCALARS = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t,
            "double": ctypes.c_double}
_MIRRORS = {"isac_carrier": "Carrier", "isac_est_params": "EstParams", "isac_cfar_config": "CfarConfig", "isac_radar_channel_params": "RadarChannelParams",
            "isac_music2d_params": "Music2dParams", "isac_est_result": "EstResult", "isac_csi_report": "CsiReport", "isac_srs_report": "SrsReport",
            "isac_cdl_job": "CdlJob", "isac_sensing_job": "SensingJob", "isac_rx_frontend_job": "RxFrontendJob", "isac_path_loss_config": "PathLossConfig"}
_RETURNS = {"int": ctypes.c_int, "const char*": ctypes.c_char_p}


def _header_without_comments():
    hdr = open(os.path.join(ROOT, "include", "isac.h")).read()
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S))


def _header_prototypes():
    """[(return type, name, [parameter type, ...])] of every function include/isac.h declares; `T name[n]` is the pointer `T*`."""
    out = []
    for ret, name, params in re.findall(r"\b(int|const char\s*\*)\s+(isac_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _header_without_comments()):
        types = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            m = re.fullmatch(r"(.*?)\s*\b\w+\s*(\[\d*\])?", " ".join(p.split()))
            types.append(re.sub(r"\s*\*", "*", m.group(1)) + ("*" if m.group(2) else ""))
        out.append((re.sub(r"\s*\*", "*", ret), name, types))
    return out


def _rule(c_type, L):
    if "*" not in c_type:
        return _SCALARS[c_type]
    m = re.fullmatch(r"(?:const )?(isac_\w+)\*", c_type)
    return ctypes.POINTER(getattr(L, _MIRRORS[m.group(1)])) if m and m.group(1) in _MIRRORS else ctypes.c_void_p


def test_prototype_table_matches_the_header(lib_path):
    L = load_pkg()._lib
    protos = _header_prototypes()
    hdr = open(os.path.join(ROOT, "include", "isac.h")).read()
    assert len(protos) == 77 == len(set(re.findall(r"\b(isac_[a-z0-9_]+)\s*\(", hdr)) - {"isac_status"})      # the regex found every declaration
    assert [name for _, name, _ in protos] == list(L.PROTOTYPES) == list(L.EXPORTS)                              # same names, in the header's order
    for ret, name, types in protos:
        restype, argtypes = L.PROTOTYPES[name]
        assert restype is _RETURNS[ret], name
        assert len(argtypes) == len(types), name
        for i, (got, c_type) in enumerate(zip(argtypes, types)):
            assert got is _rule(c_type, L), f"{name} argument {i}: {c_type}"
    lib = L.load()
    for name, (restype, argtypes) in L.PROTOTYPES.items():                                                       # and load() applied the table
        fn = getattr(lib, name)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name


def test_option_and_status_constants_match_the_header():
    L = load_pkg()._lib
    hdr = _header_without_comments()
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
