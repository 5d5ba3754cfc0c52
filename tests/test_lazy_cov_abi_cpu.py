"""include/isac_lazy_cov.h without a GPU: additive under ABI 8 and included by isac.h; its two functions are exported and carry their lines in PROTOTYPES_LAZY_COV (re-derived here
from the header by the typing rule of tests/test_abi_cpu.py), its two route constants are the binding's, and the tables of isac.h and of the older additive headers -- the
isac_ctx_set_option options among them -- are as they were."""
from __future__ import annotations

import ctypes
import os
import re

import pytest

from conftest import ROOT, load_pkg


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    return load_pkg()._lib


def test_header_against_the_binding(L):
    hdr = open(os.path.join(ROOT, "include", "isac_lazy_cov.h")).read()
    main = open(os.path.join(ROOT, "include", "isac.h")).read()
    assert '#include "isac_lazy_cov.h"' in main and "LAZY_COV" not in re.sub(r"/\*.*?\*/", " ", main, flags=re.S)      # no sixth isac_ctx_set_option option
    plain = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    protos = re.findall(r"\bint\s+(isac_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", plain)
    assert [n for n, _ in protos] == list(L.PROTOTYPES_LAZY_COV) == ["isac_ctx_set_lazy_cov_route", "isac_ctx_get_lazy_cov_route_used"]
    scal = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32}
    plain = re.sub(r"\bint32_t\s*\*", "int32_t* ", plain)
    lib = L.load()                                                             # (needs no GPU) load() applied the line
    for name, params in protos:
        want = []
        for p in params.split(","):
            m = re.fullmatch(r"(.*?)\s*\b\w+", " ".join(p.split()))
            t = re.sub(r"\s*\*", "*", m.group(1))
            want.append(scal[t] if "*" not in t else ctypes.c_void_p)
        assert L.PROTOTYPES_LAZY_COV[name] == (ctypes.c_int, tuple(want)) and len(want) == 2, name
        assert all(name not in tab for tab in (L.PROTOTYPES, L.PROTOTYPES_ADDED, L.PROTOTYPES_CFAR, L.PROTOTYPES_CFAR_MC))
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and tuple(fn.argtypes) == tuple(want), name
    consts = {n: int(v) for n, v in re.findall(r"\bISAC_LAZY_COV_(\w+) = (\d+)", plain)}
    assert consts == {"SPLIT": L.LAZY_COV_SPLIT, "REGENERATE": L.LAZY_COV_REGENERATE} == {"SPLIT": 0, "REGENERATE": 1}
    assert lib.isac_abi_version() == 8 == L.ISAC_ABI_VERSION and lib.isac_abi_sizeof(13) == -1                           # no new selector
    assert len(L.PROTOTYPES) == 77 and list(L.PROTOTYPES_CFAR_MC) == ["isac_cfar_monte_carlo"]
    assert sorted(n for n in dir(L) if n.startswith("OPT_")) == ["OPT_CDL_SHARE_SPECTRA", "OPT_MUSIC_ROUTE", "OPT_TAIL_FUSION", "OPT_UPA_DOA", "OPT_WIDE_ORDER"]
    assert lib.isac_ctx_get_lazy_cov_route_used(None, None) == 1
    assert lib.isac_ctx_set_lazy_cov_route(None, 0) == 1                       # refused before anything touches a device: no context (ISAC_ERR_INVALID_ARG)
