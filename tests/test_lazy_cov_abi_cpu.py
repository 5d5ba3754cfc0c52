"""include/isac_lazy_cov.h without a GPU: additive under ABI 8; its two route constants are the binding's, it adds no isac_ctx_set_option option and no isac_abi_sizeof
selector, and its two functions refuse a NULL context.  (Their prototype lines are compared with the header by tests/test_abi_cpu.py, row "isac_lazy_cov.h".)"""
from __future__ import annotations

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
    assert "LAZY_COV" not in re.sub(r"/\*.*?\*/", " ", main, flags=re.S)       # no sixth isac_ctx_set_option option
    plain = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    lib = L.load()                                                             # (needs no GPU)
    consts = {n: int(v) for n, v in re.findall(r"\bISAC_LAZY_COV_(\w+) = (\d+)", plain)}
    assert consts == {"SPLIT": L.LAZY_COV_SPLIT, "REGENERATE": L.LAZY_COV_REGENERATE} == {"SPLIT": 0, "REGENERATE": 1}
    assert lib.isac_abi_version() == 8 == L.ISAC_ABI_VERSION and lib.isac_abi_sizeof(13) == -1                           # no new selector
    assert sorted(n for n in dir(L) if n.startswith("OPT_")) == ["OPT_CDL_SHARE_SPECTRA", "OPT_MUSIC_ROUTE", "OPT_TAIL_FUSION", "OPT_UPA_DOA", "OPT_WIDE_ORDER"]
    assert lib.isac_ctx_get_lazy_cov_route_used(None, None) == 1
    assert lib.isac_ctx_set_lazy_cov_route(None, 0) == 1                       # refused before anything touches a device: no context (ISAC_ERR_INVALID_ARG)
