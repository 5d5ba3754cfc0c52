"""include/isac_track.h restated in NumPy, parametrised by dtype: numpy.longdouble is the reference of tests/test_gpu_track.py, float64 the conditioning probe of
tests/test_track_cpu.py.  The banks of a state are independent and are stepped in lock-step (arrays [B x ...]) only to keep the reference quick: nothing crosses a bank.
For every scan `step` returns the full outputs and the decision MARGINS:
    ("round", d2 [n], gap [n])   per greedy round with at least two competing pairs (track and measurement both still free), the smallest d^2 and the gap to the next
    ("gate",  d2 [n], gap [n])   per group, every (live track, measurement) pair's d^2 and its distance |d^2 - gate^2| from the gate
This module owns the scenes the GPU test runs (SCENES / scene(name) / reference(name, dtype))."""
from __future__ import annotations

from functools import lru_cache
from types import SimpleNamespace

import numpy as np

LD = np.longdouble
DEFAULTS = dict(sigmaAcc=1.0, gate=4.0, confirmHits=3, tentMisses=1, maxMisses=3, initV0=30.0)
INT_FIELDS = ("status", "id", "age", "hits", "misses", "dof")
NAN = float("nan")


def rad2deg(dtype):
    return dtype(57.29577951308232087679815481410517) if dtype is np.float64 else LD(180) / (LD(4) * np.arctan(LD(1)))


def new_state(B, T, dtype=LD):
    z = lambda *s: np.zeros((B, T) + s, dtype=np.int64)                      # noqa: E731
    return SimpleNamespace(B=B, T=T, dtype=dtype, status=z(), id=z(), age=z(), hits=z(), misses=z(), dof=z(), x=np.zeros((B, T, 4), dtype=dtype),
                           P=np.zeros((B, T, 4, 4), dtype=dtype), nis=np.zeros((B, T), dtype=dtype), next_id=np.zeros(B, dtype=np.int64))


def _sym(P):
    return (P + np.swapaxes(P, -1, -2)) * P.dtype.type(0.5)


def predict(x, P, dt, q):
    """Step 1 on x [.. x 4], P [.. x 4 x 4]."""
    x = x.copy()
    x[..., 0] = x[..., 0] + dt * x[..., 2]
    x[..., 1] = x[..., 1] + dt * x[..., 3]
    A = P.copy()
    A[..., 0, :] = P[..., 0, :] + dt * P[..., 2, :]
    A[..., 1, :] = P[..., 1, :] + dt * P[..., 3, :]
    N = A.copy()
    N[..., :, 0] = A[..., :, 0] + dt * A[..., :, 2]
    N[..., :, 1] = A[..., :, 1] + dt * A[..., :, 3]
    dt2 = dt * dt
    q4, q3, q2 = q * (dt2 * dt2 / 4), q * (dt2 * dt / 2), q * dt2
    for i, j, v in ((0, 0, q4), (1, 1, q4), (0, 2, q3), (2, 0, q3), (1, 3, q3), (3, 1, q3), (2, 2, q2), (3, 3, q2)):
        N[..., i, j] = N[..., i, j] + v
    return x, _sym(N)


def component(x, P, H, nu, var, on):
    """One scalar component where `on`: (x, P, nu^2 / s or 0)."""
    with np.errstate(all="ignore"):
        PH = ((P[..., :, 0] * H[0][..., None] + P[..., :, 1] * H[1][..., None]) + P[..., :, 2] * H[2][..., None]) + P[..., :, 3] * H[3][..., None]
        s = (((H[0] * PH[..., 0] + H[1] * PH[..., 1]) + H[2] * PH[..., 2]) + H[3] * PH[..., 3]) + var
        K = PH / s[..., None]
        xn = x + K * nu[..., None]
        Pn = _sym(P - K[..., :, None] * PH[..., None, :])
        d2 = nu * nu / s
    return np.where(on[..., None], xn, x), np.where(on[..., None, None], Pn, P), np.where(on, d2, d2.dtype.type(0))


def _geom(x, pt, pr, height):
    a = [x[..., 0] - pt[..., 0], x[..., 1] - pt[..., 1], height - pt[..., 2]]
    b = [x[..., 0] - pr[..., 0], x[..., 1] - pr[..., 1], height - pr[..., 2]]
    da, db = np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]), np.sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2])
    with np.errstate(all="ignore"):
        zero = da.dtype.type(0)
        gx = np.where(da != 0, a[0] / da, zero) + np.where(db != 0, b[0] / db, zero)
        gy = np.where(da != 0, a[1] / da, zero) + np.where(db != 0, b[1] / db, zero)
    return gx, gy, da + db


def apply(x, P, m, height, valid):
    """Step 3: the measurements m (kind, z [.. x 4], var [.. x 4], pt, pr [.. x 3], all broadcast to x's leading shape) applied where `valid`: (x, P, d2, components)."""
    dtype = x.dtype.type
    zero = np.zeros(x.shape[:-1], dtype=dtype)
    d2, n = zero.copy(), np.zeros(x.shape[:-1], dtype=np.int64)
    k0, k1 = valid & (m["kind"] == 0), valid & (m["kind"] == 1)
    if k0.any():
        for c in range(4):
            on = k0 & ~np.isnan(m["z"][..., c])
            H = [zero + (1 if j == c else 0) for j in range(4)]
            x, P, d = component(x, P, H, m["z"][..., c] - x[..., c], m["var"][..., c], on)
            d2, n = d2 + d, n + on
    if k1.any():
        k = rad2deg(dtype)
        gx, gy, rs = _geom(x, m["pt"], m["pr"], height)
        x, P, d = component(x, P, [gx, gy, zero, zero], m["z"][..., 0] - rs, m["var"][..., 0], k1)
        d2, n = d2 + d, n + k1
        ex, ey = x[..., 0] - m["pr"][..., 0], x[..., 1] - m["pr"][..., 1]
        e2 = ex * ex + ey * ey
        on = k1 & ~np.isnan(m["z"][..., 1]) & (e2 != 0)
        if on.any():
            with np.errstate(all="ignore"):
                w = m["z"][..., 1] - np.arctan2(ey, ex) * k
                nu = w - 360 * np.floor((w + 180) / 360)
                H = [k * -ey / e2, k * ex / e2, zero, zero]
            x, P, d = component(x, P, H, nu, m["var"][..., 1], on)
            d2, n = d2 + d, n + on
        on = k1 & ~np.isnan(m["z"][..., 2])
        gx, gy, rs = _geom(x, m["pt"], m["pr"], height)
        x, P, d = component(x, P, [zero, zero, -gx, -gy], m["z"][..., 2] + (x[..., 2] * gx + x[..., 3] * gy), m["var"][..., 2], on)
        d2, n = d2 + d, n + on
    return x, P, d2, n


def sort_records(records):
    """Per bank: (the record's fields sorted stably by group, the order)."""
    out = []
    for r in records:
        g = np.asarray(r["group"], dtype=np.int64).reshape(-1)
        o = np.argsort(g, kind="stable")
        out.append((dict(group=g[o], kind=np.asarray(r["kind"], dtype=np.int64).reshape(-1)[o], link=np.asarray(r["link"], dtype=np.int64).reshape(-1)[o],
                         z=np.asarray(r["z"], dtype=np.float64).reshape(-1, 4)[o], sigma=np.asarray(r["sigma"], dtype=np.float64).reshape(-1, 4)[o]), o))
    return out


def step(st, nodes, links, height, par, records, dt):
    """One scan of every bank of `st` (changed in place).  records: one per bank, in the caller's order.  Returns the outputs (the table copied, assoc / assoc_kind per bank
    in the caller's order, n_confirmed) with .margins."""
    dtype, B, T = st.dtype, st.B, st.T
    nodes, links, height, dt = np.asarray(nodes, dtype=dtype).reshape(-1, 3), np.asarray(links, dtype=np.int64).reshape(-1, 2), dtype(height), dtype(dt)
    q, gate2, v02 = dtype(par["sigmaAcc"]) ** 2, dtype(par["gate"]) ** 2, dtype(par["initV0"]) ** 2
    recs = sort_records(records)
    live0 = st.status > 0
    xp, Pp = predict(st.x, st.P, dt, q)
    st.x, st.P = np.where(live0[..., None], xp, st.x), np.where(live0[..., None, None], Pp, st.P)
    st.nis[:], st.dof[:] = 0, 0
    got = np.zeros((B, T), dtype=bool)
    assoc = [np.full(len(r["group"]), -1, dtype=np.int64) for r, _ in recs]
    kind_out = [np.zeros(len(r["group"]), dtype=np.int64) for r, _ in recs]
    margins = []
    L = int(live0.sum(axis=1).max()) if B else 0
    slots = np.full((B, max(L, 1)), -1, dtype=np.int64)                      # the live slots of a bank, ascending, padded
    for b in range(B):
        s = np.flatnonzero(live0[b])
        slots[b, :s.size] = s
    t_ok, sl = slots >= 0, np.maximum(slots, 0)
    bi = np.arange(B)[:, None]
    for g in sorted(set(int(v) for r, _ in recs for v in r["group"])) if L else []:
        idx = [np.flatnonzero(r["group"] == g) for r, _ in recs]
        Mg = max(i.size for i in idx)
        mi = np.full((B, Mg), -1, dtype=np.int64)
        for b in range(B):
            mi[b, :idx[b].size] = idx[b]
        m_ok = mi >= 0
        gather = lambda f, shape, dt_: np.stack([np.concatenate([np.asarray(recs[b][0][f][idx[b]], dtype=dt_), np.zeros((Mg - idx[b].size,) + shape, dtype=dt_)]) for b in range(B)])   # noqa: E731
        z, sg, kd, lk = gather("z", (4,), dtype), gather("sigma", (4,), dtype), gather("kind", (), np.int64), gather("link", (), np.int64)
        m = dict(kind=kd[:, None, :], z=z[:, None, :, :], var=(sg * sg)[:, None, :, :], pt=nodes[links[lk, 0]][:, None, :, :], pr=nodes[links[lk, 1]][:, None, :, :])
        pair_ok = t_ok[:, :, None] & m_ok[:, None, :]
        shape = (B, slots.shape[1], Mg)
        x0 = np.broadcast_to(st.x[bi, sl][:, :, None, :], shape + (4,))
        P0 = np.broadcast_to(st.P[bi, sl][:, :, None, :, :], shape + (4, 4))
        Xv, Pv, D, Nv = apply(x0, P0, m, height, pair_ok)                       # the virtual update of every pair: the real one of the pair taken is the same arithmetic
        with np.errstate(invalid="ignore"):
            margins.append(("gate", D[pair_ok], np.abs(D[pair_ok] - gate2)))
            cand = pair_ok & (D <= gate2)
        t_free, m_free = t_ok.copy(), m_ok.copy()
        while True:
            free = t_free[:, :, None] & m_free[:, None, :]
            Dc = np.where(free & cand, D, np.inf).reshape(B, -1)
            pick = Dc.argmin(axis=1)                                         # the first of equal minima: the lower slot, then the lower measurement
            has = np.isfinite(Dc[np.arange(B), pick])
            if not has.any():
                break
            Da = np.partition(np.where(free & pair_ok, D, np.inf).reshape(B, -1), 1, axis=1)[:, :2] if D[0].size > 1 else np.full((B, 1), np.inf)
            if Da.shape[1] == 2:
                two = has & np.isfinite(Da[:, 1])
                margins.append(("round", Da[two, 0], Da[two, 1] - Da[two, 0]))
            bb = np.flatnonzero(has)
            ti, mj = pick[bb] // Mg, pick[bb] % Mg
            ts = slots[bb, ti]
            st.x[bb, ts], st.P[bb, ts] = Xv[bb, ti, mj], Pv[bb, ti, mj]
            st.nis[bb, ts] += D[bb, ti, mj]
            st.dof[bb, ts] += Nv[bb, ti, mj]
            got[bb, ts] = True
            t_free[bb, ti], m_free[bb, mj] = False, False
            for b, t, j in zip(bb, ts, mj):
                assoc[b][mi[b, j]], kind_out[b][mi[b, j]] = t, 1
    # ---- bookkeeping and births
    for b in range(B):
        lv = live0[b]
        st.age[b][lv] += 1
        st.hits[b][lv & got[b]] += 1
        st.misses[b][lv & got[b]] = 0
        st.misses[b][lv & ~got[b]] += 1
        st.status[b][(st.status[b] == 1) & (st.hits[b] >= par["confirmHits"])] = 2
        st.status[b][((st.status[b] == 1) & (st.misses[b] >= par["tentMisses"])) | ((st.status[b] == 2) & (st.misses[b] >= par["maxMisses"]))] = 0
        r = recs[b][0]
        for j in np.flatnonzero((r["kind"] == 0) & (assoc[b] < 0)):
            free = np.flatnonzero(st.status[b] == 0)
            if free.size == 0:
                kind_out[b][j] = 3
                continue
            t = int(free[0])
            zj, have = r["z"][j].astype(dtype), ~np.isnan(r["z"][j])
            st.x[b, t] = np.where(have, zj, dtype(0))
            st.P[b, t] = np.diag(np.where(have, r["sigma"][j].astype(dtype) ** 2, v02))
            st.status[b, t], st.hits[b, t], st.misses[b, t], st.age[b, t], st.nis[b, t], st.dof[b, t] = 1, 1, 0, 1, 0, 0
            st.next_id[b] += 1
            st.id[b, t] = st.next_id[b]
            assoc[b][j], kind_out[b][j] = t, 2
    out = SimpleNamespace(**{k: getattr(st, k).copy() for k in INT_FIELDS + ("x", "P", "nis")}, n_confirmed=(st.status == 2).sum(axis=1), margins=margins)
    out.assoc, out.assoc_kind = [], []
    for b, (_, o) in enumerate(recs):
        for dst, src in ((out.assoc, assoc[b]), (out.assoc_kind, kind_out[b])):
            a = np.empty(o.size, dtype=np.int64)
            a[o] = src
            dst.append(a)
    return out


def run(sc, dtype=LD):
    """The scene's scans from a reset state: the list of step()'s outputs."""
    st = new_state(sc.B, sc.T, dtype)
    return [step(st, sc.nodes, sc.links, sc.height, sc.par, records, dt) for dt, records in sc.scans]


# ---------------------------------------------------------------- records and scenes
def record(rows):
    """rows: (group, kind, link, z [4], sigma [4]) each."""
    rows = list(rows)
    return dict(group=np.array([r[0] for r in rows], dtype=np.int32), kind=np.array([r[1] for r in rows], dtype=np.int32), link=np.array([r[2] for r in rows], dtype=np.int32),
                z=np.array([r[3] for r in rows], dtype=np.float64).reshape(-1, 4), sigma=np.array([r[4] for r in rows], dtype=np.float64).reshape(-1, 4))


def fix(x, y, vx=NAN, vy=NAN, group=0, sp=1.0, sv=0.5):
    return (group, 0, 0, [x, y, vx, vy], [sp, sp, sv, sv])


def link_row(k, r, azi=NAN, s=NAN, group=None, sr=1.0, sa=1.0, sv=0.5):
    return (1 + k if group is None else group, 1, k, [r, azi, s, 0.0], [sr, sa, sv, 1.0])


NODES3 = np.array([[0.0, 0.0, 25.0], [800.0, 0.0, 25.0], [400.0, 700.0, 30.0]])


def all_links(n):
    return np.array([(t, r) for r in range(n) for t in range(n)], dtype=np.int32)


def exact_link(nodes, links, k, p, v, height):
    """(range sum, azimuth seen from the rx node, Doppler sum) of the point p = (x, y) moving with v = (vx, vy), in float64."""
    pt, pr = nodes[links[k][0]], nodes[links[k][1]]
    q = np.array([p[0], p[1], height])
    a, b = q - pt, q - pr
    da, db = np.linalg.norm(a), np.linalg.norm(b)
    g = a[:2] / da + b[:2] / db
    return da + db, np.degrees(np.arctan2(b[1], b[0])), -(v[0] * g[0] + v[1] * g[1])


def _scene(name, B, T, scans, nodes=NODES3, links=None, height=1.5, exact_ties=0, **par):
    return SimpleNamespace(name=name, B=B, T=T, nodes=np.asarray(nodes, dtype=np.float64), links=all_links(len(nodes)) if links is None else np.asarray(links, dtype=np.int32),
                           height=height, par={**DEFAULTS, **par}, scans=scans, exact_ties=exact_ties)


def _minimum():
    """B = 1, T = 1, one fix a scan: birth, confirmation at the third hit, a scan with dt = 0, three misses (a far fix that finds the table full) and deletion, rebirth."""
    rng = np.random.default_rng(101)
    scans, t = [], 0.0
    for i in range(14):
        dt = 0.0 if i in (0, 5) else 0.5
        t += dt
        p = np.array([100.0 + 8.0 * t, 50.0 - 3.0 * t]) + rng.normal(0, 1.0, 2)
        if i in (8, 9, 10):
            p = p + 500.0
        scans.append((dt, [record([fix(p[0], p[1])])]))
    return _scene("b1_t1_m1", 1, 1, scans)


def _three_in_a_group():
    """B = 1, T = 2, three fixes in one group: more measurements than tracks, the third finds the table full; from scan 6 on one target is gone, its track dies and the
    clutter fix of that scan is born into the slot it leaves."""
    rng = np.random.default_rng(102)
    scans = []
    for i in range(12):
        t = 0.5 * i
        rows = [fix(*(np.array([300.0 + 5.0 * t, 200.0 + 2.0 * t]) + rng.normal(0, 1.0, 2)), *(np.array([5.0, 2.0]) + rng.normal(0, 0.5, 2)))]
        if i < 6:
            rows.append(fix(*(np.array([500.0 - 6.0 * t, 400.0]) + rng.normal(0, 1.0, 2))))
        rows.append(fix(*rng.uniform(0.0, 800.0, 2)))
        scans.append((0.5, [record(rows)]))
    return _scene("b1_t2_m3", 1, 2, scans)


def _full_table():
    """B = 1, T = 256: 256 fixes in one group fill the table; then 256 and one more in a second group (table full); all confirmed at the third scan; from scan 3 only the
    first 40 are seen and the other 216 are deleted together at max_misses, into slots that later clutter takes."""
    rng = np.random.default_rng(103)
    gx, gy = np.meshgrid(np.arange(16) * 60.0, np.arange(16) * 60.0)
    p0 = np.column_stack([gx.ravel(), gy.ravel()]) + rng.uniform(-5, 5, (256, 2))
    v = rng.uniform(-4, 4, (256, 2))
    scans = []
    for i in range(12):
        t = 0.5 * i
        p = p0 + v * t + rng.normal(0, 1.0, (256, 2))
        order = rng.permutation(256)
        rows = [fix(p[j, 0], p[j, 1]) for j in (order if i < 3 else order[order < 40])]
        if i >= 1:
            rows.append(fix(*rng.uniform(1000.0, 1500.0, 2), group=1))
        scans.append((0.5, [record(rows)]))
    return _scene("b1_t256_full", 1, 256, scans)


def _link_rows(nodes, links, height, p, v, rng, ks, azimuth=True, doppler=True, sr=1.0, sa=1.0, sv=0.5):
    rows = []
    for k in ks:
        r, a, s = exact_link(nodes, links, k, p, v, height)
        a = (a + rng.normal(0, sa) + 180.0) % 360.0 - 180.0
        rows.append(link_row(k, r + rng.normal(0, sr), a if azimuth else NAN, s + rng.normal(0, sv) if doppler else NAN, sr=sr, sa=sa, sv=sv))
    return rows


def _empty_banks_and_groups():
    """B = 3, T = 16.  Bank 0: two targets, fixes for three scans, then links only.  Bank 1: the same with M = 0 in scans 4, 5, 6 and 9 (the tracks coast, one run of three
    misses deletes them).  Bank 2: its fixes in group 7 and its links in groups 40 and 200, nothing in between; records given unsorted."""
    rng = np.random.default_rng(104)
    links = all_links(3)
    tg = [(np.array([250.0, 300.0]), np.array([6.0, -3.0])), (np.array([520.0, 260.0]), np.array([-5.0, 4.0]))]
    scans = []
    for i in range(13):
        t = 0.5 * i
        banks = []
        for b in range(3):
            rows = []
            for p0, v in tg:
                p = p0 + v * t
                if i < 3 or i % 5 == 0:
                    rows.append(fix(*(p + rng.normal(0, 1.0, 2)), *(v + rng.normal(0, 0.5, 2)), group=7 if b == 2 else 0))
                if i >= 2:
                    ks = (1, 5) if b == 2 else (0, 3, 4, 7)
                    lr = _link_rows(NODES3, links, 1.5, p, v, rng, ks, azimuth=(b == 0))
                    rows += [(40 if r[2] == 1 else 200,) + r[1:] for r in lr] if b == 2 else lr
            if b == 1 and i in (4, 5, 6, 9):
                rows = []
            if b == 2:
                rows = [rows[j] for j in rng.permutation(len(rows))]
            banks.append(record(rows))
        scans.append((0.5, banks))
    return _scene("b3_t16_empty", 3, 16, scans)


def _many_banks():
    """B = 64, T = 64, three nodes, nine links x 16 measurements a scan (10 targets, Pd 0.9 per link, the rest false measurements) and fixes mixed in: all of them in the
    first three scans, a third of them afterwards, 30 % of them without a velocity, and one false fix a scan (with a velocity, so that its gate is narrow and it dies)."""
    rng = np.random.default_rng(105)
    links = all_links(3)
    scans, Q = [], 10
    p0 = rng.uniform([100.0, 100.0], [700.0, 600.0], (64, Q, 2))
    v = rng.uniform(-8.0, 8.0, (64, Q, 2))
    for i in range(12):
        t = 0.4 * i
        banks = []
        for b in range(64):
            rows = []
            for j in range(Q):
                p = p0[b, j] + v[b, j] * t
                if i < 3 or rng.random() < 0.33:
                    has_v = rng.random() < 0.7
                    rows.append(fix(*(p + rng.normal(0, 1.0, 2)), *((v[b, j] + rng.normal(0, 0.5, 2)) if has_v else (NAN, NAN))))
            rows.append(fix(*rng.uniform(0.0, 800.0, 2), *rng.uniform(-8.0, 8.0, 2)))
            for k in range(9):
                lr = []
                for j in range(Q):
                    if rng.random() < 0.9:
                        lr += _link_rows(NODES3, links, 1.5, p0[b, j] + v[b, j] * t, v[b, j], rng, (k,), azimuth=False)
                while len(lr) < 16:
                    lr.append(link_row(k, rng.uniform(600.0, 2200.0), NAN, rng.uniform(-20.0, 20.0)))
                rows += [lr[j] for j in rng.permutation(16)]
            banks.append(record(rows))
        scans.append((0.4, banks))
    return _scene("b64_t64_links", 64, 64, scans)


def _ties():
    """Dyadic inputs, dt = 0: two tracks born at (0, 0) and (8, 0) with unit sigmas; then one fix at (4, 0) in group 0 -- d^2 = 16 / 2 = 8 from both, the lower slot takes it
    -- and the fixes (8, 4) and (8, -4) in group 1 -- d^2 = 8 from slot 1 to both, the lower measurement is taken, the other is born.  Noisy scans follow."""
    rng = np.random.default_rng(106)
    scans = [(0.0, [record([fix(0.0, 0.0), fix(8.0, 0.0)])]),
             (0.0, [record([fix(8.0, 4.0, group=1), fix(4.0, 0.0), fix(8.0, -4.0, group=1)])])]
    for i in range(11):
        t = 0.5 * (i + 1)
        rows = [fix(*(np.array([2.0 + 3.0 * t, 1.0 * t]) + rng.normal(0, 1.0, 2))), fix(*(np.array([8.0 + 2.0 * t, 2.0 + 4.0 * t]) + rng.normal(0, 1.0, 2))),
                fix(*(np.array([8.0 - 1.0 * t, -4.0 - 5.0 * t]) + rng.normal(0, 1.0, 2)))]
        scans.append((0.5, [record(rows)]))
    return _scene("ties", 1, 4, scans, exact_ties=2, initV0=32.0)


def _special():
    """B = 1, T = 8.  Slot 0: a track exactly on node 2's vertical (born from a dyadic fix at rest, dt = 0), given the mono-static link 8 = (2, 2) with azimuth and Doppler: g = 0, the
    range row is zero, the azimuth is skipped, u is formed at height 1.5 under the node at 30.  Slot 1: a target west of node 1 crossing azimuth +-180 seen from it, the
    measured azimuth on the other side of the cut from the predicted one.  Slots 2, 3: fixes and links with vx / vy and azimuth / Doppler NaN in every combination."""
    rng = np.random.default_rng(107)
    links = all_links(3)
    scans = []
    pw0, vw = np.array([500.0, 0.4]), np.array([2.0, -0.4])                  # west of node 1 (800, 0): azimuth 180 -+ a little, y crossing 0
    pc0, vc = np.array([300.0, 350.0]), np.array([4.0, 3.0])
    pd0, vd = np.array([600.0, 450.0]), np.array([-3.0, 5.0])
    combos = [(a, b) for a in (False, True) for b in (False, True)]
    for i in range(13):
        dt = 0.0 if i == 1 else 0.5
        t = 0.5 * max(i - 1, 0)
        rows = []
        if i == 0:
            rows.append(fix(400.0, 700.0, 0.0, 0.0))                         # at rest: its velocity is never observed (g = 0), so it has to be given
        else:
            rows.append(link_row(8, 2.0 * 28.5 + rng.normal(0, 0.5), 33.0, rng.normal(0, 0.5), sr=1.0))
        pw = pw0 + vw * t
        if i < 3:
            rows.append(fix(*(pw + rng.normal(0, 0.5, 2)), *(vw + rng.normal(0, 0.3, 2)), sp=0.5, sv=0.3))
        else:
            r, a, s = exact_link(NODES3, links, 4, pw, vw, 1.5)              # link 4 = (1, 1): mono-static at node 1
            a = a + (0.3 if i % 2 else -0.3)
            rows.append(link_row(4, r + rng.normal(0, 0.5), (a + 180.0) % 360.0 - 180.0, s + rng.normal(0, 0.3), sr=0.5, sa=0.5, sv=0.3))
            r, a, s = exact_link(NODES3, links, 0, pw, vw, 1.5)
            rows.append(link_row(0, r + rng.normal(0, 0.5), NAN, s + rng.normal(0, 0.3), sr=0.5, sv=0.3))
        for p0, v, shift in ((pc0, vc, 0), (pd0, vd, 1)):
            p = p0 + v * t
            hx, hy = combos[(i + shift) % 4]
            vm = v + rng.normal(0, 0.5, 2)
            rows.append(fix(*(p + rng.normal(0, 1.0, 2)), vm[0] if hx else NAN, vm[1] if hy else NAN))
            if i >= 1:
                for k, (az, dp) in zip((1, 3, 0, 4), combos):               # links between nodes 0 and 1: no ellipse of theirs passes through node 2
                    rows += _link_rows(NODES3, links, 1.5, p, v, rng, (k,), azimuth=az, doppler=dp)
        scans.append((dt, [record(rows)]))
    return _scene("special", 1, 8, scans, sigmaAcc=0.25)                      # (a small process noise keeps the track at rest from growing into the others' range ellipses)


SCENES = {"b1_t1_m1": _minimum, "b1_t2_m3": _three_in_a_group, "b1_t256_full": _full_table, "b3_t16_empty": _empty_banks_and_groups, "b64_t64_links": _many_banks,
          "ties": _ties, "special": _special}


@lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


@lru_cache(maxsize=None)
def reference(name, dtype=LD):
    """The scene's outputs scan by scan; computed once and shared, so leave it unchanged."""
    return run(scene(name), dtype)
