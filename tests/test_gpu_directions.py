"""isac_resolve_directions on the MI355X: off-grid direction finding with several sources per array snapshot (project-defined -- include/isac_directions.h, DESIGN.md
section 5).

Scenes and the long-double answer come from tests/_directions_restatement.py; tests/test_directions_cpu.py has shown that the restatement recovers every scene's truth and
that every box its maximiser meets holds exactly one local maximum.  Each reference is computed once per process and shared."""
from __future__ import annotations

import ctypes as C
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest

import _directions_restatement as R

pytestmark = pytest.mark.gpu

LOBE_TOL = 1e-6        # |dir_dev - dir_ref| x (elements on the axis) x d: the project's NU_TOL, a millionth of a lobe
FIELD_TOL = 1e-10      # the project's field tolerance
FLOOR = 1e-12          # as tests/test_directions_cpu.py
SENTINEL = -7
OUT = ("status", "n_found", "n_src", "azi", "ele", "dir_u", "dir_v", "power", "amp", "residual")


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context()
    yield c
    c.close()


def _ep(pkg, upa):
    return pkg._lib.EstParams(512, 64, 1.0, 1.0, 0 if upa is None else 1, 0 if upa is None else upa[0], 0 if upa is None else upa[1], 360.0, 1.0, 180.0, 1.0)


def _raw(pkg, c, x, upa=None, K=1, cycles=16, min_ratio=0.01, min_power=0.0, A=None, n=None, ep=True, null=()):
    """The C call itself: (status code, namespace of the raw outputs, pre-filled with a sentinel)."""
    x = np.asfortranarray(np.asarray(x, dtype=np.complex128))
    A = x.shape[0] if A is None else A
    n = x.shape[1] if n is None else n
    m, kk = max(x.shape[1], 1), max(K, 1)
    o = SimpleNamespace(status=np.full(m, SENTINEL, dtype=np.int32), n_found=np.full(m, SENTINEL, dtype=np.int32), n_src=np.full(m, SENTINEL, dtype=np.int32),
                        residual=np.full(m, float(SENTINEL)), amp=np.full((kk, m), SENTINEL, dtype=np.complex128, order="F"))
    for k in ("azi", "ele", "dir_u", "dir_v", "power"):
        setattr(o, k, np.full((kk, m), float(SENTINEL), order="F"))
    p = lambda name: None if name in null else getattr(o, name).ctypes.data_as(C.c_void_p)   # noqa: E731
    e = _ep(pkg, upa)
    st = c.lib.isac_resolve_directions(c.handle, C.byref(e) if ep else None, None if "snapshots" in null else x.ctypes.data_as(C.c_void_p), A, n, K, cycles, min_ratio,
                                       min_power, p("status"), p("n_found"), p("n_src"), p("azi"), p("ele"), p("dir_u"), p("dir_v"), p("power"), p("amp"), p("residual"))
    return st, o


def _same(a, b, cols=None):
    for k in OUT:
        u, v = getattr(a, k), getattr(b, k)
        if cols is not None:
            u, v = u[..., cols[0]], v[..., cols[1]]
        assert np.ascontiguousarray(u).tobytes() == np.ascontiguousarray(v).tobytes(), k


def _untouched(o):
    return all((getattr(o, k) == SENTINEL).all() for k in OUT)


_runs = {}


def _run(pkg, c, name, K=None):
    key = (name, K)
    if key not in _runs:
        s = R.scene(name)
        st, o = _raw(pkg, c, s.x, s.upa, s.K if K is None else K)
        assert st == 0, c.lib.isac_last_error(c.handle)
        _runs[key] = o
    return _runs[key]


def _against(s, dev, ref):
    """The comparison with the restatement: counts and order exact, accepted sources to LOBE_TOL / FIELD_TOL."""
    g = s.geom
    assert np.array_equal(dev.status, ref.status) and np.array_equal(dev.n_found, ref.n_found) and np.array_equal(dev.n_src, ref.n_src)
    worst = 0.0
    for i in range(dev.status.size):
        norm = (np.abs(s.x[:, i]) ** 2).sum() / s.A
        assert abs(dev.residual[i] - ref.residual[i]) <= FIELD_TOL * norm
        for k in range(ref.n_src[i]):
            e = R.lobes(g, dev.dir_u[k, i] - ref.dir_u[k, i], (dev.dir_v[k, i] - ref.dir_v[k, i]) if g.two_d else 0.0)
            worst = max(worst, e)
            assert e <= LOBE_TOL, (i, k, e)
            assert abs(dev.power[k, i] / ref.power[k, i] - 1.0) <= FIELD_TOL and abs(dev.amp[k, i] - ref.amp[k, i]) <= FIELD_TOL * abs(ref.amp[k, i])
            assert dev.power[k, i] == dev.amp[k, i].real ** 2 + dev.amp[k, i].imag ** 2
        for k in range(ref.n_found[i], dev.power.shape[0]):                # the slots behind the sources found
            assert np.isnan(dev.dir_u[k, i]) and np.isnan(dev.power[k, i]) and np.isnan(dev.azi[k, i]) and dev.amp[k, i] == 0
    return worst


def _angles(s, dev):
    """azi / ele are the principal-branch degrees of dir_u / dir_v to 1e-12 degrees."""
    for i in range(dev.status.size):
        for k in range(dev.n_found[i]):
            u, v = dev.dir_u[k, i], dev.dir_v[k, i]
            if s.geom.two_d:
                assert abs(dev.ele[k, i] - np.degrees(np.arcsin(min(1.0, np.hypot(u, v))))) <= 1e-12 and 0.0 <= dev.ele[k, i] <= 90.0
                assert abs(dev.azi[k, i] - np.degrees(np.arctan2(v, u))) <= 1e-12
            else:
                assert abs(dev.azi[k, i] - np.degrees(np.arcsin(u))) <= 1e-12 and -90.0 <= dev.azi[k, i] <= 90.0
                assert dev.dir_v[k, i] == SENTINEL and dev.ele[k, i] == SENTINEL   # a ULA: not written


@pytest.mark.parametrize("name", list(R.SINGLE))
def test_single_source(pkg, ctx, name):
    """ULA A = 2, 4, 16, 64, 256 and UPA 2 x 8, 8 x 2, 4 x 4, 16 x 16, n = 1 and 5: against the restatement and, noise-free, against the truth to 1e-6 of a lobe."""
    s, dev, ref = R.scene(name), _run(pkg, ctx, name), R.reference(name)
    worst = _against(s, dev, ref)
    _angles(s, dev)
    truth = max(R.truth_error(s, dev, i)[0] for i in range(s.n))
    print(f"{name}: {worst:.3e} lobes off the restatement, {truth:.3e} off the truth; residual {dev.residual.max():.3e}")
    assert truth <= LOBE_TOL


@pytest.mark.parametrize("name", list(R.MULTI))
def test_two_and_three_sources(pkg, ctx, name):
    """max_sources = 2 and 3: strongest first, every source within the bound tests/test_directions_cpu.py recorded for the restatement plus 1e-6 of a lobe."""
    s, dev, ref = R.scene(name), _run(pkg, ctx, name), R.reference(name)
    worst = _against(s, dev, ref)
    _angles(s, dev)
    truth = max(R.truth_error(s, dev, i)[0] for i in range(s.n))
    print(f"{name}: {worst:.3e} lobes off the restatement, {truth:.3e} off the truth; residual {dev.residual.max():.3e}")
    assert (dev.n_src == s.K).all() and all((np.diff(dev.power[:, i]) <= 0).all() for i in range(s.n))
    assert truth <= max(10.0 * R.MEASURED_LOBES[name], FLOOR) + LOBE_TOL


def test_one_source_of_two_is_biased(pkg, ctx):
    """max_sources = 1 on the two-source snapshots: one source, measurably off the stronger target (the restatement says by how much) -- the cycles do something."""
    s, dev, ref = R.scene("ula16_two"), _run(pkg, ctx, "ula16_two", 1), R.reference("ula16_two", 1)
    _against(s, dev, ref)
    for i in range(s.n):
        bias = R.lobes(s.geom, dev.dir_u[0, i] - s.truth[i][0][0])
        assert dev.n_found[i] == 1 and bias >= 1e-4, (i, bias)


def test_floors(pkg, ctx):
    """A third extraction on a noise-free two-source snapshot is written (n_found = 3) and not counted (n_src = 2); min_power above the weaker source: n_src = 1."""
    s = R.scene("ula16_two")
    st, o = _raw(pkg, ctx, s.x, None, 3)
    print(f"n_found {o.n_found.tolist()} n_src {o.n_src.tolist()} power {o.power.T.tolist()}")
    assert st == 0 and (o.n_found == 3).all() and (o.n_src == 2).all() and not np.isnan(o.dir_u).any()
    two = _run(pkg, ctx, "ula16_two")
    assert np.abs(o.dir_u[:2] - two.dir_u).max() * 16 * 0.5 <= LOBE_TOL       # the third source does not disturb the two
    st, o = _raw(pkg, ctx, s.x[:, :1], None, 2, min_power=0.1)
    assert st == 0 and o.n_found.tolist() == [2] and o.n_src.tolist() == [1]
    assert o.dir_u.tobytes() == np.ascontiguousarray(two.dir_u[:, :1]).tobytes()   # the floors change the count alone


def test_degenerate_columns(pkg, ctx):
    """A zero column and a NaN column: status 1, n_src 0; their neighbours' results are byte-identical to a run without them."""
    s = R.scene("ula16_two")
    x = np.zeros((16, 4), dtype=np.complex128)
    x[:, 1], x[:, 3] = s.x[:, 0], s.x[:, 1]
    x[5, 2] = np.nan
    st, o = _raw(pkg, ctx, x, None, 2)
    assert st == 0 and o.status.tolist() == [1, 0, 1, 0] and o.n_found.tolist() == [0, 2, 0, 2] and o.n_src.tolist() == [0, 2, 0, 2]
    assert np.isnan(o.dir_u[:, [0, 2]]).all() and np.isnan(o.power[:, [0, 2]]).all() and np.isnan(o.azi[:, [0, 2]]).all() and not o.amp[:, [0, 2]].any()
    assert o.residual[0] == 0.0 and np.isnan(o.residual[2])
    _same(o, _run(pkg, ctx, "ula16_two"), cols=([1, 3], [0, 1]))
    up = R.scene("upa4x4")
    y = np.zeros((16, 3), dtype=np.complex128)
    y[:, 1] = up.x[:, 2]
    y[0, 2] = np.nan
    st, o = _raw(pkg, ctx, y, (4, 4), 1)
    assert st == 0 and o.status.tolist() == [1, 0, 1] and np.isnan(o.ele[:, [0, 2]]).all() and np.isnan(o.dir_v[:, [0, 2]]).all()
    _same(o, _run(pkg, ctx, "upa4x4"), cols=([1], [2]))


def test_determinism(pkg, ctx):
    """Two calls give byte-identical results; n = 1024 at A = 16 equals the n = 5 run on its first five entries, byte for byte."""
    s = R.scene("ula16_two")
    first = _run(pkg, ctx, "ula16_two")
    st, again = _raw(pkg, ctx, s.x, None, 2)
    assert st == 0
    _same(first, again)
    rng = np.random.default_rng(41)
    big = np.asfortranarray(np.concatenate([s.x, rng.standard_normal((16, 1019)) + 1j * rng.standard_normal((16, 1019))], axis=1))
    st, o = _raw(pkg, ctx, big, None, 2)
    assert st == 0 and (o.status == 0).all() and (o.n_found == 2).all()
    _same(o, first, cols=(slice(0, 5), slice(0, 5)))
    st, o2 = _raw(pkg, ctx, big, None, 2)
    assert st == 0
    _same(o, o2)


def test_errors(pkg, ctx):
    """Every ISAC_ERR_INVALID_ARG (1) / ISAC_ERR_UNSUPPORTED (7) case of the header; the outputs are untouched on failure; n = 0 is ISAC_OK."""
    L = pkg._lib
    x = R.scene("ula16").x
    xu = R.scene("upa4x4").x
    ok = lambda r: r[0] == 0                                                # noqa: E731
    bad = lambda r, code=1: r[0] == code and _untouched(r[1])             # noqa: E731
    assert bad(_raw(pkg, ctx, x, ep=False))
    for name in ("snapshots", "status", "n_found", "n_src", "azi", "dir_u", "power"):
        assert bad(_raw(pkg, ctx, x, null=(name,))), name
    for name in ("ele", "dir_v"):
        assert bad(_raw(pkg, ctx, xu, (4, 4), null=(name,))), name          # a planar array needs both
    assert ok(_raw(pkg, ctx, x, null=("ele", "dir_v", "amp", "residual")))   # a ULA does not; amp and residual are optional
    assert bad(_raw(pkg, ctx, x, n=-1))
    big = np.zeros((4, L.ISAC_MAX_TARGETS + 1), dtype=np.complex128, order="F")
    assert bad(_raw(pkg, ctx, big)) and ok(_raw(pkg, ctx, big[:, :-1]))
    for K in (0, -1, L.ISAC_DIR_MAX_SOURCES + 1, 16):
        assert bad(_raw(pkg, ctx, x, K=K)), K
    assert ok(_raw(pkg, ctx, x, K=L.ISAC_DIR_MAX_SOURCES)) and bad(_raw(pkg, ctx, x[:4], K=4)) and ok(_raw(pkg, ctx, x[:4], K=3))   # at most A - 1
    assert bad(_raw(pkg, ctx, x, cycles=-1)) and ok(_raw(pkg, ctx, x, K=2, cycles=0))
    for r in (-0.1, 1.5, float("nan"), float("inf")):
        assert bad(_raw(pkg, ctx, x, min_ratio=r)), r
    for p in (-1.0, float("nan"), float("inf")):
        assert bad(_raw(pkg, ctx, x, min_power=p)), p
    assert ok(_raw(pkg, ctx, x, min_ratio=0.0)) and ok(_raw(pkg, ctx, x, min_ratio=1.0))
    assert bad(_raw(pkg, ctx, x[:1])) and bad(_raw(pkg, ctx, x, A=0))       # A < 2
    for upa in ((4, 3), (3, 4), (0, 16), (16, 0), (-4, -4)):
        assert bad(_raw(pkg, ctx, xu, upa)), upa                            # n_ants_x n_ants_y != A
    wide = np.ones((257, 1), dtype=np.complex128, order="F")
    assert bad(_raw(pkg, ctx, wide), 7) and bad(_raw(pkg, ctx, wide, (257, 1)), 7)
    st, o = _raw(pkg, ctx, x[:, :0])
    assert st == 0 and _untouched(o)                                        # n = 0
    with pytest.raises(pkg.IsacError) as e:
        pkg.sensing.estimation.resolveDirections(ctx, SimpleNamespace(nIFFT=512, nFFT=64, rRes=1.0, vRes=1.0, azimuthScanScale=360, azimuthScanGranularity=1,
                                                                      elevationScanScale=180, elevationScanGranularity=1), x, maxSources=0)
    assert e.value.name == "INVALID_ARG"


def test_python_rows(pkg, ctx):
    """sensing.estimation.resolveDirections on arrays: rows = the accepted sources of the C call in entry order; twin changes degrees alone; a UPA carries ele."""
    rp = SimpleNamespace(nIFFT=512, nFFT=64, rRes=1.0, vRes=1.0, azimuthScanScale=360, azimuthScanGranularity=1, elevationScanScale=180, elevationScanGranularity=1)
    s, raw = R.scene("ula16_two"), _run(pkg, ctx, "ula16_two")
    f = pkg.sensing.estimation.resolveDirections
    d = f(ctx, rp, s.x, maxSources=2)
    assert d["entry"].tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4] and d["src"].tolist() == [0, 1] * 5 and "ele" not in d and "rng" not in d
    assert d["dir_u"].tobytes() == raw.dir_u.T.tobytes() and d["azi"].tobytes() == raw.azi.T.tobytes() and d["amp"].tobytes() == raw.amp.T.tobytes()
    assert np.array_equal(d["n_src"], raw.n_src) and d["residual"].tobytes() == raw.residual.tobytes()
    one = f(ctx, rp, dict(snapshots=s.x, rng=np.arange(5.0), vel=-np.arange(5.0), row=np.arange(5), col=np.arange(5) + 7), maxSources=2, minPower=0.1, twin=True)
    assert one["entry"].tolist() == [0, 1, 1, 2, 2, 3, 3, 4] and one["rng"].tolist() == [0.0, 1.0, 1.0, 2.0, 2.0, 3.0, 3.0, 4.0] and one["col"][0] == 7   # powers 0.04 and 0.09 fall below 0.1
    keep = [0, 2, 3, 4, 5, 6, 7, 8]
    assert one["dir_u"].tobytes() == d["dir_u"][keep].tobytes()
    t = 180.0 - d["azi"][keep]
    assert np.array_equal(one["azi"], np.where(t > 180.0, t - 360.0, t))
    up = R.scene("upa4x4")
    rpu = SimpleNamespace(antennaType=SimpleNamespace(kind="upa", nV=4, nH=4), **vars(rp))
    du, dt = f(ctx, rpu, up.x), f(ctx, rpu, up.x, twin=True)
    ru = _run(pkg, ctx, "upa4x4")
    assert du["ele"].tobytes() == ru.ele[0].tobytes() and du["dir_v"].tobytes() == ru.dir_v[0].tobytes() and np.array_equal(dt["ele"], -du["ele"])
    assert np.abs(np.abs(dt["azi"] - du["azi"]) - 180.0).max() <= 1e-12 and dt["dir_u"].tobytes() == du["dir_u"].tobytes()
    quadrants = {(a > 0, abs(a) > 90) for a in du["azi"]}
    assert len(quadrants) == 4                                              # the scene covers all four azimuth quadrants


# ---------------------------------------------------------------- end to end: the capability itself
def _chain(pkg, c, name):
    """monoStaticSensing -> fft2D -> targetList(snapshots=True) of an end-to-end scene, then every getter before and after resolveDirections."""
    sc = R.make_e2e(name)
    est_mod = pkg.sensing.estimation
    F = import_module(pkg.__name__ + ".sensing.estimation.fft2D")
    rp = pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)
    cf = pkg.sensing.detection.cfar2D(rp)
    d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
    echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c)
    est_mod.fft2D(rp, cf, echo, d_txg, ctx=c)
    before = SimpleNamespace(tl=est_mod.targetList(c, snapshots=True), dbg=F.fft2D_debug(c, sc.A))
    res = est_mod.resolveDirections(c, rp, before.tl, maxSources=len(R.E2E[name]["velocity"]))
    after = SimpleNamespace(tl=est_mod.targetList(c, snapshots=True), dbg=F.fft2D_debug(c, sc.A))
    rf = est_mod.refineTargets(c, before.tl, snapshots=True)
    est_mod.resolveDirections(c, rp, rf, maxSources=2)                     # a refined list is accepted as well
    rf_after = est_mod.refineTargets(c, before.tl, snapshots=True)
    for d in (echo, d_txg, d_wave):
        d.free()
    for k in ("row", "col", "hits", "power", "rng", "vel", "azi", "snapshots"):
        assert before.tl[k].tobytes() == after.tl[k].tobytes(), k
    for k in ("power_window", "Ra", "spectrum_db"):
        assert getattr(before.dbg, k).tobytes() == getattr(after.dbg, k).tobytes(), k
    for a, b in zip(before.dbg.detections + before.dbg.det_pow, after.dbg.detections + after.dbg.det_pow):
        assert a.tobytes() == b.tobytes()
    for k in ("nu", "vel", "azi", "power", "status", "snapshots"):
        assert rf[k].tobytes() == rf_after[k].tobytes(), k
    return sc, before.tl, res


def test_two_targets_in_one_cell(pkg, ctx):
    """Two targets at the same range and velocity, azimuths 10.4 and 40.7 degrees: the list holds ONE entry for the cell, with one integer azimuth; resolveDirections
    returns two rows for it, each within 0.1 degrees (in sind) of a target and within 1e-6 of a lobe of the restatement on the oracle's snapshot; the getters, the list and
    a following refineTargets answer byte for byte as before."""
    p = R.oracle_e2e("pair")
    sc, tl, res = _chain(pkg, ctx, "pair")
    assert np.array_equal(tl["row"], p.list.row) and np.array_equal(tl["col"], p.list.col)
    cell = np.flatnonzero((tl["row"] == tl["row"][0]) & (tl["col"] == tl["col"][0]))
    assert cell.size == 1 and float(tl["azi"][0]).is_integer()
    rows = np.flatnonzero(res["entry"] == 0)
    err = [float(R.u_distance(res["dir_u"][r], p.truth_u).min()) for r in rows]
    near = sorted(int(R.u_distance(res["dir_u"][r], p.truth_u).argmin()) for r in rows)
    print(f"list azi {tl['azi'].tolist()}; resolved dir_u {res['dir_u'][rows].tolist()}, truth {p.truth_u.tolist()}, errors {err}")
    assert rows.size == 2 and near == [0, 1] and max(err) <= np.sin(np.radians(0.1))
    assert np.abs(res["dir_u"][rows] - p.ref.dir_u[:, 0]).max() * sc.A * 0.5 <= LOBE_TOL
    assert np.array_equal(res["rng"][rows], np.full(2, tl["rng"][0])) and np.array_equal(res["vel"][rows], np.full(2, tl["vel"][0]))
    rm = pkg.sensing.postProcessing.getRMSE(res, pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave))   # getRMSE takes the result as it stands
    assert rm.rngRMSE.size == res["rng"].size and np.isfinite(rm.rngRMSE[rows]).all()


def test_single_target_off_the_grid(pkg, ctx):
    """One target at 10.4 degrees: the resolved direction is closer to the target than the list's grid azimuth (in sind)."""
    q = R.oracle_e2e("single")
    sc, tl, res = _chain(pkg, ctx, "single")
    fine = float(R.u_distance(res["dir_u"][0], q.truth_u[0]))
    grid = float(R.u_distance(np.sin(np.radians(tl["azi"][0])), q.truth_u[0]))
    print(f"list azi {tl['azi'][0]}: grid error {grid:.3e}, resolved error {fine:.3e} in sind")
    assert res["entry"][0] == 0 and fine < grid
    assert abs(res["dir_u"][0] - q.ref.dir_u[0, 0]) * sc.A * 0.5 <= LOBE_TOL
