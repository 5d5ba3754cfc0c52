"""Target tracking across CPIs without a GPU (include/isac_track.h): the restatement of tests/_track_restatement.py against textbook algebra and on exact
scenes, the conditioning of every scene tests/test_gpu_track.py compares the device on, the binding's lines for the stand-alone header, and the host helpers.
  1. kind-0 sequential scalar updates equal the joint Kalman update, and the summed d^2 the joint Mahalanobis distance, to 1e-12
  2. fixes on exact constant-velocity trajectories keep every track on the truth to 1e-9 m
  3. a track started by three scans of fixes is kept by two links alone, in scans in which the localiser (minLinks = 3) reports nothing
  4. every device scene: float64 and long double make the same integer decisions, agree to 1e-10 in x and to 1e-10 of the largest |P| in P, and every decision margin
     is at least 1e4 times the float64-vs-long-double discrepancy of its d^2 and at least 1e-9 relative; the scenes provoke what they are for
  5. the lines of _lib.TRACK_PROTOTYPES re-derived from the header; isac_track_state_bytes at the limits; every refusal against the CPU-loaded library
  6. trackMeasurements and getTrackRMSE on hand-made inputs"""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np
import pytest

import _abi_header as H
import _localize_restatement as RL
import _track_restatement as R
from conftest import load_pkg

X_MAX = 1e-10
P_MAX = 1e-10
DECIDABLE = 1e4
REL_MIN = 1e-9


# ---------------------------------------------------------------- 1
def test_sequential_scalar_updates_equal_the_joint_kalman_update():
    rng = np.random.default_rng(5)
    worst = [0.0, 0.0, 0.0]
    for _ in range(20):
        A = rng.normal(size=(4, 4))
        P = A @ A.T + 0.1 * np.eye(4)
        P = (P + P.T) / 2
        x, z, sig = rng.normal(size=4) * 10, rng.normal(size=4) * 10, rng.uniform(0.3, 3.0, 4)
        m = dict(kind=np.zeros(1, dtype=np.int64), z=z[None], var=(sig ** 2)[None], pt=np.zeros((1, 3)), pr=np.zeros((1, 3)))
        xs, Ps, d2, n = R.apply(x[None].copy(), P[None].copy(), m, np.float64(0.0), np.ones(1, dtype=bool))
        S = P + np.diag(sig ** 2)                                           # H = I, R diagonal
        K = P @ np.linalg.inv(S)
        xj, Pj, dj = x + K @ (z - x), P - K @ P, float((z - x) @ np.linalg.solve(S, z - x))
        worst = [max(worst[0], np.abs(xs[0] - xj).max() / np.abs(xj).max()), max(worst[1], np.abs(Ps[0] - Pj).max() / np.abs(Pj).max()), max(worst[2], abs(d2[0] - dj) / dj)]
        assert n[0] == 4 and np.array_equal(Ps[0], Ps[0].T)
    print(f"sequential vs joint, relative: x {worst[0]:.2e}, P {worst[1]:.2e}, d^2 vs Mahalanobis {worst[2]:.2e}")
    assert max(worst) <= 1e-12


# ---------------------------------------------------------------- 2
def test_noiseless_fixes_keep_tracks_on_the_truth():
    p0 = np.array([[210.5, 310.25], [523.75, 188.5], [390.25, 455.0], [655.5, 402.75]])
    v = np.array([[10.0, -3.0], [-7.0, 12.0], [0.0, 15.0], [-20.0, -5.0]])
    st = R.new_state(1, 8)
    worst = 0.0
    for i in range(12):
        t = 0.5 * i
        rec = R.record([R.fix(*(p0[j] + v[j] * t), *v[j]) for j in (2, 0, 3, 1)])
        o = R.step(st, R.NODES3, R.all_links(3), 1.5, R.DEFAULTS, [rec], 0.5)
        assert o.assoc[0].tolist() == [0, 1, 2, 3] and o.id[0, :4].tolist() == [1, 2, 3, 4]
        assert (o.status[0, :4] == (2 if i >= 2 else 1)).all() and (o.status[0, 4:] == 0).all()
        if i >= 2:
            truth = np.hstack([p0 + v * t, v])[[2, 0, 3, 1]]
            worst = max(worst, float(np.abs(o.x[0, :4] - truth).max()))
    print(f"noiseless fixes: largest state error after confirmation {worst:.3e}")
    assert worst <= 1e-9


# ---------------------------------------------------------------- 3
def test_two_links_keep_a_track_the_localiser_drops():
    rng = np.random.default_rng(9)
    nodes, links = R.NODES3, R.all_links(3)
    p0, v, sr, sv = np.array([310.0, 260.0]), np.array([8.0, -5.0]), 1.0, 0.5
    st = R.new_state(1, 4)
    two = (0, 4)                                                            # the mono-static links of nodes 0 and 1
    g = []
    for k in two:
        pt, pr = nodes[links[k][0]], nodes[links[k][1]]
        q = np.array([p0[0], p0[1], 1.5])
        g.append((q - pt)[:2] / np.linalg.norm(q - pt) + (q - pr)[:2] / np.linalg.norm(q - pr))
    J = np.array(g) / sr
    bound = 4.0 * float(np.sqrt(np.linalg.eigvalsh(np.linalg.inv(J.T @ J)).max()))   # four sigma of ONE scan's two-link position fix; the track also has its prediction
    errs = []
    for i in range(8):
        t = 0.5 * i
        p = p0 + v * t
        if i < 3:
            rec = R.record([R.fix(*(p + rng.normal(0, 1.0, 2)))])
        else:
            rows = R._link_rows(nodes, links, 1.5, p, v, rng, two, azimuth=False, sr=sr, sv=sv)
            rec = R.record(rows)
            meas = dict(link=rec["link"], r=rec["z"][:, 0], s=rec["z"][:, 2], azi=rec["z"][:, 1], sigma_r=rec["sigma"][:, 0], sigma_v=rec["sigma"][:, 2], sigma_a=rec["sigma"][:, 1])
            sc = RL.make_scene(nodes, [tuple(l) for l in links], meas, (p[0] - 40.0, 2.0, 41, p[1] - 40.0, 2.0, 41), 1.5)
            assert len(RL.localize(sc, RL.position_map(sc), **RL.DEFAULTS).pos) == 0     # two links: the localiser has nothing to say
        o = R.step(st, nodes, links, 1.5, R.DEFAULTS, [rec], 0.5)
        errs.append(float(np.hypot(*(o.x[0, 0, :2].astype(np.float64) - p))))
        if i >= 2:
            assert o.status[0, 0] == 2 and o.id[0, 0] == 1 and o.n_confirmed[0] == 1
        if i >= 3:
            assert o.assoc[0].tolist() == [0, 0] and o.dof[0, 0] == 4
    print(f"link-only maintenance: errors {errs} m; bound {bound:.3f} m (four sigma of a single scan's two-link fix, sigma_r {sr} m)")
    assert max(errs[3:]) <= bound


# ---------------------------------------------------------------- 4
def _events(ref):
    """What happened in a run: confirmations, deletions, a slot reused inside a scan, kinds seen."""
    ev = dict(confirm_at_hits=set(), tent_deleted=0, conf_deleted=0, reused=0, kinds=set(), ids_ok=True)
    prev, given = None, np.zeros(ref[0].id.shape[0], dtype=np.int64)        # the ids a bank has given so far
    for o in ref:
        ev["kinds"] |= set(int(v) for a in o.assoc_kind for v in a)
        if prev is not None:
            conf = (prev.status == 1) & (o.status == 2) & (o.id == prev.id)
            ev["confirm_at_hits"] |= set(o.hits[conf].tolist())
            gone = (prev.status > 0) & ((o.status == 0) | (o.id != prev.id))
            ev["tent_deleted"] += int((gone & (prev.status == 1)).sum())
            ev["conf_deleted"] += int((gone & (prev.status == 2)).sum())
            ev["reused"] += int(((prev.status > 0) & (o.status > 0) & (o.id != prev.id)).sum())
        for b in range(o.id.shape[0]):                                      # every id born in this scan is live at its end: the next ones, without a gap
            new = np.sort(o.id[b][(o.status[b] > 0) & (o.id[b] > given[b])])
            ev["ids_ok"] &= new.tolist() == list(range(given[b] + 1, given[b] + 1 + new.size))
            given[b] += new.size
        prev = o
    return ev


@pytest.mark.parametrize("name", list(R.SCENES))
def test_device_scenes_are_well_conditioned(name):
    sc, ref, f64 = R.scene(name), R.reference(name), R.reference(name, np.float64)
    assert len(ref) >= 12
    ex = ep = 0.0
    worst_ratio, worst_rel, zero_gaps = np.inf, np.inf, 0
    for a, b in zip(ref, f64):
        for k in R.INT_FIELDS + ("n_confirmed",):
            assert np.array_equal(getattr(a, k), getattr(b, k)), k
        for u, w in zip(a.assoc + a.assoc_kind, b.assoc + b.assoc_kind):
            assert np.array_equal(u, w)
        ex = max(ex, float(np.abs(a.x - b.x.astype(R.LD)).max()))
        ep = max(ep, float(np.abs(a.P - b.P.astype(R.LD)).max() / max(float(np.abs(a.P).max()), 1e-300)))
        assert np.array_equal(a.P, np.swapaxes(a.P, -1, -2)) and np.array_equal(b.P, np.swapaxes(b.P, -1, -2))   # exactly symmetric
        assert len(a.margins) == len(b.margins)
        for (kind, d2, gap), (kind_b, d2_b, gap_b) in zip(a.margins, b.margins):
            assert kind == kind_b and d2.shape == d2_b.shape
            if not d2.size:
                continue
            disc = np.abs(d2 - d2_b.astype(R.LD)).astype(np.float64)
            gap, scale = gap.astype(np.float64), np.maximum(d2.astype(np.float64), float(sc.par["gate"]) ** 2 if kind == "gate" else 0.0)
            tie = gap == 0.0
            zero_gaps += int(tie.sum())
            if (~tie).any():
                with np.errstate(divide="ignore"):
                    worst_ratio = min(worst_ratio, float((gap[~tie] / disc[~tie]).min()))
                    worst_rel = min(worst_rel, float((gap[~tie] / scale[~tie]).min()))
    ev = _events(ref)
    print(f"{name}: float64 vs long double: x {ex:.3e}, P {ep:.3e} of its largest entry; smallest margin {worst_ratio:.3e} discrepancies, {worst_rel:.3e} relative; "
          f"{zero_gaps} exact ties; events {ev}")
    assert ex <= X_MAX and ep <= P_MAX
    assert zero_gaps == sc.exact_ties                                       # only the scene built to tie ties, and exactly where it was built to
    assert worst_ratio >= DECIDABLE and worst_rel >= REL_MIN
    assert ev["ids_ok"]
    want = {"b1_t1_m1": dict(kinds={1, 2, 3}, conf_deleted=1, tent_deleted=1, reused=1), "b1_t2_m3": dict(kinds={1, 2, 3}, conf_deleted=1, tent_deleted=1, reused=1),
            "b1_t256_full": dict(kinds={1, 2, 3}, conf_deleted=216), "b3_t16_empty": dict(kinds={0, 1, 2}, conf_deleted=2), "b64_t64_links": dict(kinds={0, 1, 2}, tent_deleted=1),
            "ties": dict(kinds={1, 2}), "special": dict(kinds={1, 2})}[name]
    assert ev["kinds"] >= want["kinds"] and ev["confirm_at_hits"] == {sc.par["confirmHits"]}
    for k in ("conf_deleted", "tent_deleted", "reused"):
        assert ev[k] >= want.get(k, 0), k


def test_special_scenes_hold_what_they_are_for():
    ref = R.reference("ties")
    assert ref[0].assoc[0].tolist() == [0, 1] and ref[1].assoc[0].tolist() == [1, 0, 2] and ref[1].assoc_kind[0].tolist() == [1, 1, 2]   # lower slot; lower measurement; the other born
    assert float(ref[1].nis[0, 0]) == 8.0 and float(ref[1].nis[0, 1]) == 8.0 and ref[1].x[0, 0].tolist() == [2.0, 0.0, 0.0, 0.0]
    sc, ref = R.scene("special"), R.reference("special")
    assert sc.scans[1][0] == 0.0 and R.scene("b1_t1_m1").scans[5][0] == 0.0                                      # dt = 0
    for o in ref[1:]:                                                       # slot 0 sits exactly on node 2's vertical: the azimuth is skipped (range and Doppler: 2 components)
        assert o.x[0, 0, :2].tolist() == [400.0, 700.0] and o.dof[0, 0] == 2 and o.status[0, 0] > 0
    wrapped = 0
    for (dt, recs), o in zip(sc.scans, ref):                                # slot 1: measured azimuths on both sides of the cut, the track on one
        az = recs[0]["z"][(recs[0]["kind"] == 1) & (recs[0]["link"] == 4), 1]
        if az.size and o.dof[0, 1] == 5:
            pred = np.degrees(np.arctan2(float(o.x[0, 1, 1]), float(o.x[0, 1, 0]) - 800.0))
            wrapped += abs(az[0] - pred) > 180.0
    assert wrapped >= 2
    z = np.vstack([r[0]["z"][r[0]["kind"] == 0] for _, r in sc.scans])
    assert {(bool(np.isnan(a)), bool(np.isnan(b))) for a, b in z[:, 2:]} == {(False, False), (False, True), (True, False), (True, True)}
    z = np.vstack([r[0]["z"][r[0]["kind"] == 1] for _, r in sc.scans])
    assert {(bool(np.isnan(a)), bool(np.isnan(b))) for a, b in z[:, 1:3]} == {(False, False), (False, True), (True, False), (True, True)}
    sc = R.scene("b3_t16_empty")
    assert any(len(r[1]["group"]) == 0 for _, r in sc.scans) and set(np.concatenate([r[2]["group"] for _, r in sc.scans]).tolist()) == {7, 40, 200}
    assert any(not np.array_equal(r[2]["group"], np.sort(r[2]["group"])) for _, r in sc.scans)                    # given unsorted: the wrapper's stable sort is exercised
    sc = R.scene("b1_t256_full")
    assert [len(r[0]["group"]) for _, r in sc.scans][:3] == [256, 257, 257] and (R.reference("b1_t256_full")[1].assoc_kind[0] == 3).sum() == 1
    sc = R.scene("b64_t64_links")
    assert all(((r["group"] == 1 + k) & (r["kind"] == 1)).sum() == 16 for _, recs in sc.scans for r in recs for k in range(9))


# ---------------------------------------------------------------- 5
@pytest.fixture(scope="module")
def lib_path():
    import __graft_entry__ as g
    g.build()
    p = load_pkg().library_path()
    assert os.path.exists(p)
    return p


def test_track_prototypes_match_the_header(lib_path):
    L = load_pkg()._lib
    header = "isac_track.h"
    assert list(L.TRACK_PROTOTYPES) == [header] and header not in H.includes() and not any(header in t for t in (L.HEADER_PROTOTYPES, L.STANDALONE_PROTOTYPES, L.LOCALIZE_PROTOTYPES))
    assert re.search(r'^#include "isac\.h"', H.text(header), flags=re.M) and "isac_track.h" not in H.text("isac.h")
    protos = H.prototypes(header)                                           # the `int` functions; the size query returns int64_t and is parsed here
    m = re.search(r"\bint64_t\s+(isac_track_state_bytes)\s*\(([^()]*)\)\s*;", H.without_comments(header))
    assert m and [" ".join(p.split()[:-1]) for p in m.group(2).split(",")] == ["int32_t", "int32_t"]
    table = L.TRACK_PROTOTYPES[header]
    assert list(table) == ["isac_track_state_bytes"] + [name for _, name, _ in protos] and not set(table) & set(L.PROTOTYPES)
    assert table["isac_track_state_bytes"] == (ctypes.c_int64, (ctypes.c_int32, ctypes.c_int32))
    assert [(name, len(types)) for _, name, types in protos] == [("isac_track_reset_dev", 4), ("isac_track_step_dev", 35), ("isac_track_get_dev", 13)]
    for ret, name, types in protos:
        restype, argtypes = table[name]
        assert restype is H.RETURNS[ret], name
        assert len(argtypes) == len(types), name
        for i, (got, c_type) in enumerate(zip(argtypes, types)):
            assert got is H.rule(c_type, L), f"{name} argument {i}: {c_type}"
    assert protos[1][2][23:32] == protos[2][2][4:13]                        # the same table in the step and in the getter
    raw = ctypes.CDLL(lib_path)
    assert all(hasattr(raw, name) for name in table)
    lib = L.load()
    for name, (restype, argtypes) in table.items():                         # and load() applied the table
        fn = getattr(lib, name)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name
    assert int(re.search(r"#define ISAC_ABI_VERSION (\d+)", H.text("isac.h")).group(1)) == 8 == L.ISAC_ABI_VERSION
    for name in ("MAX_BANKS", "MAX_TRACKS", "MAX_GROUPS", "MAX_GROUP_MEAS", "MAX_MEAS", "MAX_NODES", "MAX_LINKS"):
        v = re.search(rf"#define ISAC_TRACK_{name} (\(1 << (\d+)\)|\d+)", H.text(header))
        assert (1 << int(v.group(2)) if v.group(2) else int(v.group(1))) == getattr(L, "ISAC_TRACK_" + name)


def test_state_bytes_at_the_limits(lib_path):
    lib = load_pkg()._lib.load()
    f = lib.isac_track_state_bytes
    per_slot = 6 * 4 + (4 + 16 + 1) * 8                                     # six integers, x, P and nis
    assert f(1, 1) >= per_slot + 4 and f(1024, 256) >= 1024 * 256 * per_slot + 4 * 1024 and f(1024, 256) < 1024 * 256 * per_slot + (1 << 16)
    assert f(1024, 256) % 256 == 0 and f(2, 3) >= f(1, 3) and f(3, 256) > f(3, 255)
    for B, T in ((0, 1), (1, 0), (1025, 1), (1, 257), (-1, 4), (4, -1)):
        assert f(B, T) == 0, (B, T)


def _valid_call():
    """A valid isac_track_step_dev call but for the NULL context (argument 0): B = 2, T = 4, three nodes, two links, bank 0 with three measurements and bank 1 with none."""
    a = dict(nodes=np.array([[0.0, 0.0, 25.0], [80.0, 0.0, 25.0], [40.0, 64.0, 30.0]]), ltx=np.array([0, 2], dtype=np.int32), lrx=np.array([1, 2], dtype=np.int32),
             first=np.array([0, 3, 3], dtype=np.int32), group=np.array([0, 0, 1], dtype=np.int32), kind=np.array([0, 0, 1], dtype=np.int32), link=np.array([0, 0, 1], dtype=np.int32),
             z=np.array([[10.0, 20.0, np.nan, 1.0], [30.0, 40.0, 2.0, np.nan], [100.0, np.nan, np.nan, 0.0]]), sigma=np.ones((3, 4)))
    outs = {k: np.zeros(n, dtype=dt) for k, n, dt in (("status", 8, np.int32), ("id", 8, np.int32), ("age", 8, np.int32), ("hits", 8, np.int32), ("misses", 8, np.int32),
                                                       ("x", 32, np.float64), ("P", 128, np.float64), ("nis", 8, np.float64), ("dof", 8, np.int32), ("assoc", 3, np.int32),
                                                       ("assoc_kind", 3, np.int32), ("n_confirmed", 2, np.int32))}
    state = np.zeros(4096, dtype=np.uint8)                                  # never reached: every call here is refused before any device work
    p = lambda v: v.ctypes.data_as(ctypes.c_void_p)                         # noqa: E731
    args = [None, p(state), 2, 4, p(a["nodes"]), 3, p(a["ltx"]), p(a["lrx"]), 2, 1.5, 0.5, 1.0, 4.0, 3, 1, 3, 30.0, p(a["first"]), p(a["group"]), p(a["kind"]), p(a["link"]),
            p(a["z"]), p(a["sigma"])] + [p(v) for v in outs.values()]
    return args, a, outs, state


# name -> ({argument index: value}, {(array, flat element): value}); argument indices as in include/isac_track.h, 0 = ctx
TRACK_REFUSALS = {
    "banks_0": ({2: 0}, {}), "banks_1025": ({2: 1025}, {}), "tracks_0": ({3: 0}, {}), "tracks_257": ({3: 257}, {}), "nodes_0": ({5: 0}, {}), "nodes_65": ({5: 65}, {}),
    "links_0": ({8: 0}, {}), "links_257": ({8: 257}, {}), "height_nan": ({9: np.nan}, {}), "dt_negative": ({10: -0.5}, {}), "dt_inf": ({10: np.inf}, {}),
    "sigma_acc_negative": ({11: -1.0}, {}), "sigma_acc_nan": ({11: np.nan}, {}), "gate_inf": ({12: np.inf}, {}), "confirm_hits_0": ({13: 0}, {}), "tent_misses_0": ({14: 0}, {}),
    "max_misses_0": ({15: 0}, {}), "init_v0_nan": ({16: np.nan}, {}),
    "node_nan": ({}, {("nodes", 4): np.nan}), "link_tx_out_of_range": ({}, {("ltx", 1): 3}), "link_rx_negative": ({}, {("lrx", 0): -1}),
    "bank_first_not_zero": ({}, {("first", 0): 1}), "bank_first_descending": ({}, {("first", 1): 3, ("first", 2): 2}), "bank_first_above_2_20": ({}, {("first", 2): (1 << 20) + 1}),
    "group_negative": ({}, {("group", 0): -1}), "group_256": ({}, {("group", 2): 256}), "group_not_ascending": ({}, {("group", 0): 1, ("group", 1): 0}),
    "kind_2": ({}, {("kind", 1): 2}), "link_out_of_range": ({}, {("link", 2): 2}), "link_negative": ({}, {("link", 2): -1}),
    "fix_x_nan": ({}, {("z", 0): np.nan}), "fix_vx_inf": ({}, {("z", 2): np.inf}), "r_nan": ({}, {("z", 8): np.nan}), "azi_inf": ({}, {("z", 9): np.inf}), "s_inf": ({}, {("z", 10): -np.inf}),
    "sigma_zero": ({}, {("sigma", 5): 0.0}), "sigma_negative": ({}, {("sigma", 0): -1.0}), "sigma_nan": ({}, {("sigma", 11): np.nan}), "sigma_inf": ({}, {("sigma", 2): np.inf}),
    **{f"null_{i}": ({i: None}, {}) for i in (1, 4, 6, 7, 17, 18, 19, 20, 21, 22, *range(23, 35))},
}


def test_group_of_257_is_refused(lib_path):
    lib = load_pkg()._lib.load()
    args, a, outs, _ = _valid_call()
    n = 257
    big = dict(first=np.array([0, n, n], dtype=np.int32), group=np.zeros(n, dtype=np.int32), kind=np.zeros(n, dtype=np.int32), link=np.zeros(n, dtype=np.int32),
               z=np.zeros((n, 4)), sigma=np.ones((n, 4)), assoc=np.zeros(n, dtype=np.int32), assoc_kind=np.zeros(n, dtype=np.int32))
    for i, k in ((17, "first"), (18, "group"), (19, "kind"), (20, "link"), (21, "z"), (22, "sigma"), (32, "assoc"), (33, "assoc_kind")):
        args[i] = big[k].ctypes.data_as(ctypes.c_void_p)
    assert lib.isac_track_step_dev(*args) == 1


@pytest.mark.parametrize("name", list(TRACK_REFUSALS))
def test_refusals_need_no_gpu(lib_path, name):
    """Every refusal through the prototypes load() applied: ISAC_ERR_INVALID_ARG, the poisoned outputs and the state block untouched.  (The checks come before the context is
    touched; with a context the same cases run in tests/test_gpu_track.py, where the unbroken call succeeds.)"""
    lib = load_pkg()._lib.load()
    args, a, outs, state = _valid_call()
    brk, elem = TRACK_REFUSALS[name]
    for (k, e), v in elem.items():
        a[k].reshape(-1)[e] = v
    for i, v in brk.items():
        args[i] = v
    for v in outs.values():
        v[...] = -7
    state[:] = 0xA5
    assert lib.isac_track_step_dev(*args) == 1
    assert all((v == -7).all() for v in outs.values()) and (state == 0xA5).all()


def test_reset_and_get_refusals_need_no_gpu(lib_path):
    lib = load_pkg()._lib.load()
    args, _, outs, state = _valid_call()
    table = args[23:32]
    assert lib.isac_track_reset_dev(None, args[1], 2, 4) == 1 and lib.isac_track_reset_dev(None, None, 2, 4) == 1 and lib.isac_track_reset_dev(None, args[1], 0, 4) == 1
    assert lib.isac_track_get_dev(None, args[1], 2, 4, *table) == 1 and lib.isac_track_get_dev(None, args[1], 2, 257, *table) == 1
    for i in range(9):
        assert lib.isac_track_get_dev(None, args[1], 2, 4, *[None if j == i else t for j, t in enumerate(table)]) == 1
    assert (state == 0).all() and all((v == 0).all() for v in outs.values())


# ---------------------------------------------------------------- 6
def test_track_measurements_from_hand_made_inputs():
    f = load_pkg().sensing.estimation.trackMeasurements
    fixes = dict(pos=np.array([[1.0, 2.0], [3.0, 4.0]]), vel=np.array([[5.0, 6.0], [7.0, 8.0]]), vel_status=np.array([0, 1]))
    links = dict(link=np.array([2, 0], dtype=np.int32), r=np.array([100.0, 200.0]), s=np.array([1.0, np.nan]), azi=np.array([np.nan, 30.0]), sigma_r=np.array([2.0, 3.0]),
                 sigma_v=np.array([0.5, 0.6]), sigma_a=np.array([1.5, 2.5]))
    m = f(fixes, 2.0, 0.25, links)
    assert m["group"].tolist() == [0, 0, 3, 1] and m["kind"].tolist() == [0, 0, 1, 1] and m["link"].tolist() == [0, 0, 2, 0] and m["group"].dtype == np.int32
    assert m["z"][0].tolist() == [1.0, 2.0, 5.0, 6.0] and m["z"][1, :2].tolist() == [3.0, 4.0] and np.isnan(m["z"][1, 2:]).all()     # vel_status 1: no velocity
    assert m["z"][2, [0, 2, 3]].tolist() == [100.0, 1.0, 0.0] and np.isnan(m["z"][2, 1]) and m["z"][3, :2].tolist() == [200.0, 30.0] and np.isnan(m["z"][3, 2])
    assert m["sigma"].tolist() == [[2.0, 2.0, 0.25, 0.25], [2.0, 2.0, 0.25, 0.25], [2.0, 1.5, 0.5, 1.0], [3.0, 2.5, 0.6, 1.0]]
    only = f(links=links)
    assert only["kind"].tolist() == [1, 1] and only["z"].shape == (2, 4)
    assert f(fixes, 1.0, 1.0)["kind"].tolist() == [0, 0]
    none = f()
    assert none["group"].size == 0 and none["z"].shape == (0, 4) and none["sigma"].shape == (0, 4)
    with pytest.raises(ValueError):
        f(fixes)
    with pytest.raises(ValueError):
        f(links=dict(links, link=np.array([255, 0])))


def _hist(rows):
    """rows: per scan a list of (id, status, x, y, vx, vy)."""
    return [dict(tracks=[dict(id=np.array([r[0] for r in sc], dtype=np.int32), status=np.array([r[1] for r in sc], dtype=np.int32),
                              x=np.array([r[2:] for r in sc], dtype=np.float64).reshape(-1, 4))]) for sc in rows]


def test_track_rmse_on_hand_made_histories():
    f = load_pkg().sensing.postProcessing.getTrackRMSE
    truth = np.array([[[0.0, 0.0, 1.0, 0.0], [100.0, 0.0, 0.0, 2.0]], [[1.0, 0.0, 1.0, 0.0], [100.0, 2.0, 0.0, 2.0]], [[2.0, 0.0, 1.0, 0.0], [100.0, 4.0, 0.0, 2.0]],
                      [[3.0, 0.0, 1.0, 0.0], [100.0, 6.0, 0.0, 2.0]]])
    hist = _hist([[(1, 2, 0.0, 3.0, 1.0, 0.0), (2, 1, 100.0, 0.0, 0.0, 2.0)],                      # truth 0 by id 1, 3 m off; id 2 only tentative
                  [(1, 2, 1.0, 4.0, 1.0, 1.0), (2, 2, 100.0, 2.0, 0.0, 2.0), (7, 2, 500.0, 500.0, 0.0, 0.0)],   # id 7: a false confirmed track
                  [(3, 2, 2.0, 0.0, 1.0, 0.0), (2, 2, 100.0, 4.0, 0.0, 2.0), (7, 2, 500.0, 500.0, 0.0, 0.0)],   # truth 0 now by id 3: an id switch
                  [(3, 2, 3.0, 0.0, 1.0, 0.0), (2, 2, 100.0, 16.0, 0.0, 2.0)]])                    # id 2 is 10 m off: outside the gate
    r = f(hist, truth, 5.0)
    assert r.match.tolist() == [[1, 0], [1, 2], [3, 2], [3, 0]] and r.nScans.tolist() == [4, 2]
    assert r.idSwitches == 1 and r.falseTracks == 1
    assert r.posRMSE.tolist() == [np.sqrt((9.0 + 16.0) / 4.0), 0.0] and r.velRMSE.tolist() == [0.5, 0.0]
    assert f(hist, truth, 4.0).match[1].tolist() == [0, 2]                  # the gate is strict
    r = f(hist, truth[:, :, :2], 5.0)
    assert np.isnan(r.velRMSE).all() and r.posRMSE[1] == 0.0
    r = f(_hist([[], []]), truth[:2], 5.0)
    assert np.isnan(r.posRMSE).all() and r.idSwitches == 0 and r.falseTracks == 0
    with pytest.raises(ValueError):
        f(hist, truth[:3], 5.0)
