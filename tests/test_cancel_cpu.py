"""Reference-signal cancellation on the received waveform (project-defined, include/isac_cancel_paths.h) without a GPU: the restatement's own properties, the `interference`
scene of tests/_multistatic_restatement.py before and after cancellation on the oracle, sensing.channelModels.referencePaths against its restatement, the conditioning of the
edge cases tests/test_gpu_cancel.py runs, and the header and the binding's prototype line.  The device library is not asked for anything but its symbol table."""
from __future__ import annotations

import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import _cancel_restatement as X
import _multistatic_restatement as M
import _numerology_scenes as N
from conftest import ROOT, load_pkg

MARGIN = 1e-6                                                               # the bound the numerology scenes' CFAR guard margins are held to


@pytest.fixture(scope="module")
def binding():
    import __graft_entry__ as g
    g.build()
    return load_pkg()._lib


# ---------------------------------------------------------------- (a) the restatement
@pytest.mark.parametrize("name", ["t1000_a3_m9", "t4099_a3_m17"])
def test_residual_is_orthogonal_to_every_reference(name):
    """R^H Y' = 0: against |r_m| |y'_a|, at the rounding of a sum of T terms."""
    e = X.edge_case(name)
    w = e.want
    inner = np.abs(w.R.conj().T @ w.out) / (np.linalg.norm(w.R, axis=0)[:, None] * np.linalg.norm(w.out, axis=0)[None, :])
    print(f"{name}: largest normalised inner product of a reference with the residual {inner.max():.3e}; removed {10 * np.log10(w.power_in / w.power_out)} dB")
    assert inner.max() <= 1e-13
    assert (w.power_out < w.power_in).all()


def test_a_lone_zero_doppler_path_is_removed_down_to_rounding():
    """One path of the channel restatement on 3 elements, its reference with another steering scale: what is left is rounding, and the coefficients are gain x receive steering
    over the scale."""
    rng = np.random.default_rng(3)
    T = 2000
    waves = [None, np.asfortranarray(rng.standard_normal((T, 3)) + 1j * rng.standard_normal((T, 3)))]
    b, a = np.exp(2j * np.pi * rng.random(3)), np.exp(2j * np.pi * rng.random(3))
    Y = M.multi_static_channel(waves, X.FC, X.FS, 0.0, 3, [(1, 57, 0.0, 0.37, b, a)], None)
    res = X.cancel(Y, waves, X.FC, X.FS, [(1, 57, 0.0, 2.0 * b)])
    left = np.sqrt(res.power_out / res.power_in)
    print(f"residual amplitude / input amplitude per element {left}")
    assert (left <= 1e-14).all()
    assert np.abs(res.coef[0] - 0.37 * a / 2.0).max() <= 1e-14


def test_edge_cases_are_well_conditioned_and_reach_every_edge():
    seen_m, seen_a, seen_t = set(), set(), set()
    for name in X.EDGE_CASES:
        e = X.edge_case(name)
        print(f"{name}: cond(G) = {e.cond:.3g}")
        assert e.cond <= 1e3
        seen_m.add(e.M); seen_a.add(e.A); seen_t.add(e.T)
        assert e.T - 1 in e.refs.shift.tolist() and len(set(e.refs.shift.tolist())) == e.M
        if e.M > 1:
            assert 0 in e.refs.shift.tolist() and (e.refs.doppler != 0).any() and (e.refs.doppler == 0).any() and set(e.refs.source.tolist()) == {0, 1}
    assert seen_m == {1, 9, 16, 17, 32} and seen_a == {1, 3, 4} and seen_t == {1000, 4099, 30720}
    assert all(t % 256 for t in (1000, 4099))


# ---------------------------------------------------------------- (b) the interference scene on the oracle
def test_direct_path_blinds_the_cell_and_one_reference_brings_the_list_back():
    before = M.scene("interference")
    assert before.own[0] is None                                             # oracle.fft2d raises: no detection
    s = X.interference()
    sc = M.base().sc
    assert len(s.refs) == 1 and s.refs[0][0] == 1 and s.refs[0][1] == X.DIRECT_SAMPLES and s.refs[0][2] == 0.0
    removed = 10.0 * np.log10(s.res.power_in / s.res.power_out)
    print(f"removed per element {removed} dB; guard margins {['%.3g' % m for m in s.margin]}; rngEst / rRes {None if s.est is None else (s.est.rngEst / sc.rp.rRes).tolist()}")
    assert (removed > 45.0).all() and (removed < 46.0).all()
    assert all(m > MARGIN for m in s.margin)
    assert all(d.shape[1] == 3 for d in s.dets)
    assert s.est is not None
    r_res = sc.rp.rRes
    assert s.est.rngEst.tolist() == [33 * r_res, 32 * r_res, 34 * r_res]
    assert np.asarray(s.est.velEst).tolist() == [0] and np.asarray(s.est.aziEst).tolist() == [-97, -83, 90]
    clear = M.scene("bistatic").own                                          # the same scene without the direct path
    assert np.array_equal(s.est.rngEst, clear[0].rngEst) and np.array_equal(s.est.aziEst, clear[0].aziEst)
    assert all(np.array_equal(x, y) for x, y in zip(s.dets, clear[1]))


def test_five_taps_give_the_same_list():
    s1, s5 = X.interference(), X.interference(taps=2)
    assert [r[1] for r in s5.refs] == [41, 42, 43, 44, 45]
    cond = float(np.linalg.cond(s5.res.G))
    print(f"five taps: cond(G) = {cond:.4g}; guard margins {['%.3g' % m for m in s5.margin]}")
    assert cond < 200.0
    assert all(m > MARGIN for m in s5.margin)
    assert s5.est is not None and np.array_equal(s5.est.rngEst, s1.est.rngEst) and np.array_equal(s5.est.aziEst, s1.est.aziEst)
    assert all(np.array_equal(x, y) for x, y in zip(s5.dets, s1.dets))


# ---------------------------------------------------------------- (c) referencePaths
def test_reference_paths_is_its_restatement():
    pkg = load_pkg()
    b = M.base()
    sc = b.sc
    paths = pkg.sensing.channelModels.multiStaticPaths(sc.cell, [sc.cell, b.nb.cell], b.targets, carrierInfo=sc.carrier, waveInfo=sc.wave)
    assert paths.kind == X.scene_kinds()
    rows = M.path_tuples(paths)
    ref = pkg.sensing.channelModels.referencePaths
    for kinds, taps in ((("direct",), 0), (("direct",), 2), (("direct", "target"), 1), (("target",), 40), ((), 0)):
        got, want = ref(paths, kinds, taps), X.reference_paths((rows, paths.kind), kinds, taps)
        assert len(got.source) == len(want) == len(got.txSteering) == len(got.kind), (kinds, taps)
        assert got.source.dtype == np.int32 and got.shift.dtype == np.int64 and got.doppler.dtype == np.float64
        for i, (s, d, f, tb) in enumerate(want):
            assert (got.source[i], got.shift[i], got.doppler[i]) == (s, d, f) and np.array_equal(got.txSteering[i], tb)
    assert ref(paths).shift.tolist() == [X.DIRECT_SAMPLES] and ref(paths, taps=2).shift.tolist() == [41, 42, 43, 44, 45]
    assert min(ref(paths, ("target",), 40).shift.tolist()) == 0              # 33 - 40 is clipped at 0 ...
    assert ref(paths, ("target",), 40).shift.tolist().count(0) == 1          # ... once: the repeats are merged
    twice = SimpleNamespace(source=[1, 1, 1], shift=[5, 5, 5], doppler=[0.0, 0.0, 1.0], txSteering=[np.ones(2), np.ones(2), np.ones(2)], kind=[("direct", 1)] * 3)
    assert ref(twice).doppler.tolist() == [0.0, 1.0]                         # same source, shift, Doppler and steering bits: one reference
    with pytest.raises(ValueError):
        ref(paths, taps=-1)


# ---------------------------------------------------------------- (d) header and binding
def test_binding_has_the_prototype_and_the_abi_is_unchanged(binding):
    """include/isac_cancel_paths.h is additive under ABI 8: no new struct, enum or isac_abi_sizeof selector; the header states the limits, the refusals and what is out of
    scope, and its one function refuses a NULL context.  (Its prototype line is compared with the header by tests/test_abi_cpu.py, row "isac_cancel_paths.h".)"""
    L = binding
    hdr = open(os.path.join(ROOT, "include", "isac_cancel_paths.h")).read()
    plain = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    assert "typedef" not in plain and "struct" not in plain and "enum" not in plain and "ISAC_SIZEOF" not in plain
    assert int(re.search(r"#define ISAC_CANCEL_PATHS_MAX_REFS (\d+)", plain).group(1)) == 32 == L.ISAC_CANCEL_PATHS_MAX_REFS
    for word in ("OUT OF SCOPE", "MEX", "LIMITS", "n_refs 1 .. 32", "n_sources 1 .. 32", "1 .. 256", "DEPENDENT", "1e-10", "leaves d_out untouched", "*dependent = -1",
                 "ISAC_ERR_INVALID_ARG", "ISAC_ERR_CAPACITY", "launches nothing and writes nothing", "partially overlapping", "the same bits every time",
                 "cached range rows and lazy echo grid", "status record has been read back"):
        assert word in hdr, word
    lib = L.load()                                                             # (needs no GPU)
    assert lib.isac_abi_version() == 8 == L.ISAC_ABI_VERSION and lib.isac_abi_sizeof(13) == -1
    fn = lib.isac_cancel_paths_dev
    assert fn(*([None] * 3), 1, 1, 1.0, 1.0, 1, 1, *([None] * 4), 0.0, *([None] * 5)) == 1      # refused before anything touches a device: no context
    pkg = load_pkg()
    assert callable(pkg.sensing.cancelPaths) and callable(pkg.sensing.ofdmDemodulate) and callable(pkg.sensing.channelModels.referencePaths)
