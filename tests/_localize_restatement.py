"""Multi-static localisation restated in NumPy longdouble (include/isac_localize.h has the definition): stages A to C, the rounding bounds of the device's fp64 results and
the margins of every comparison whose outcome is an integer result, plus the scenes tests/test_localize_cpu.py conditions and tests/test_gpu_localize.py runs.

Bounds.  u = 2^-53.  The device forms a = rho / sigma_r from a handful of roundings of numbers no larger than R_max (the grid coordinate, two differences, the sum of
squares, two square roots, the sum, the difference with r, the product with 1 / sigma_r: under 5 u R_max / sigma_r in all) and b = alpha / sigma_a from atan2 (2 ulp at
most), the conversion to degrees, one difference, the wrap and one product (under 6 u 180 / sigma_a); C_ROUND = 8 covers both with room.  dw = w |a| da and
max_x x exp(-x^2 / 2) = 0.61, so a link's term is off by at most 0.61 C_ROUND u (R_max / sigma_r + 180 / sigma_a); exp's own ulp and the sum over K links are smaller by the
factor R_max / sigma_r.  The scenes' grid coordinates and node positions are dyadic, so x0 + ix dx is exact on the device and here."""
from __future__ import annotations

from functools import lru_cache
from types import SimpleNamespace

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
C_ROUND = 8.0
PI = 4 * np.arctan(LD(1))
R2D = LD(180) / PI
SINGULAR, VEL_COND = LD(1e-12), LD(1e-8)
DEFAULTS = dict(minScore=None, maxCand=64, minLinks=3, gate=4.0, iters=8, maxMove=None, maxTargets=64)


def wrap(d):
    return d - LD(360) * np.floor((d + LD(180)) / LD(360))


def make_scene(nodes, links, meas, grid, height):
    """meas: dict of link, r, s, azi, sigma_r, sigma_v, sigma_a in any order; the scene holds them sorted stably by link, and `order` (sorted position -> given index)."""
    link = np.asarray(meas["link"], dtype=np.int32)
    order = np.argsort(link, kind="stable")
    m = {k: np.asarray(meas[k], dtype=np.float64)[order] for k in ("r", "s", "azi", "sigma_r", "sigma_v", "sigma_a")}
    return SimpleNamespace(nodes=np.asarray(nodes, dtype=np.float64).reshape(-1, 3), links=np.asarray(links, dtype=np.int32).reshape(-1, 2), link=link[order], order=order,
                           grid=tuple(grid), height=float(height), given=meas, **m)


def grid_xy(sc):
    x0, dx, nx, y0, dy, ny = sc.grid
    return LD(x0) + np.arange(nx).astype(LD) * LD(dx), LD(y0) + np.arange(ny).astype(LD) * LD(dy)


def geom(sc, m, x, y):
    """(rho, alpha, grad rho [2], grad alpha [2]) of measurement m at (x, y) (scalars or arrays), longdouble; alpha = 0 and no gradient for a NaN azimuth."""
    tx, rx = (sc.nodes[n].astype(LD) for n in sc.links[sc.link[m]])
    z = LD(sc.height)
    et, er = (x - tx[0], y - tx[1], z - tx[2]), (x - rx[0], y - rx[1], z - rx[2])
    dt, dr = np.sqrt(et[0] ** 2 + et[1] ** 2 + et[2] ** 2), np.sqrt(er[0] ** 2 + er[1] ** 2 + er[2] ** 2)
    rho = (dt + dr) - LD(sc.r[m])
    with np.errstate(invalid="ignore", divide="ignore"):
        g_rho = (et[0] / dt + er[0] / dr, et[1] / dt + er[1] / dr)
        if np.isnan(sc.azi[m]):
            return rho, rho * 0, g_rho, (rho * 0, rho * 0)
        h2 = er[0] ** 2 + er[1] ** 2
        alpha = wrap(np.arctan2(er[1], er[0]) * R2D - LD(sc.azi[m]))
        return rho, alpha, g_rho, (-R2D * er[1] / h2, R2D * er[0] / h2)


def q_of(sc, m, x, y):
    rho, alpha, _, _ = geom(sc, m, x, y)
    return (rho / LD(sc.sigma_r[m])) ** 2 + (alpha / LD(sc.sigma_a[m])) ** 2


def position_map(sc):
    """S [ny x nx], longdouble."""
    xs, ys = grid_xy(sc)
    X, Y = np.meshgrid(xs, ys)
    S = np.zeros(X.shape, dtype=LD)
    for k in range(len(sc.links)):
        best = np.zeros(X.shape, dtype=LD)
        for m in np.flatnonzero(sc.link == k):
            best = np.maximum(best, np.exp(-q_of(sc, m, X, Y) / 2))
        S = S + best
    return S


def map_bound(sc):
    """K 0.61 c u (R_max / sigma_r,min + 180 / sigma_a,min); R_max: the largest range sum over the grid's corners, |r| and coordinate."""
    xs, ys = grid_xy(sc)
    corners = [(float(x), float(y)) for x in (xs[0], xs[-1]) for y in (ys[0], ys[-1])]
    d = lambda p, n: float(np.sqrt((p[0] - n[0]) ** 2 + (p[1] - n[1]) ** 2 + (sc.height - n[2]) ** 2))   # noqa: E731
    r_max = max([d(p, sc.nodes[t]) + d(p, sc.nodes[r]) for p in corners for t, r in sc.links] + [float(np.abs(sc.r).max())] + [abs(v) for p in corners for v in p]
                + [float(np.abs(sc.nodes).max())])
    fin = ~np.isnan(sc.azi)
    eps = C_ROUND * U * (r_max / float(sc.sigma_r.min()) + (180.0 / float(sc.sigma_a[fin].min()) if fin.any() else 0.0))
    return len(sc.links) * 0.61 * eps, eps


def candidates(S, min_score, max_cand):
    """Stage B on any map [ny x nx]: (cells, scores) of the kept candidates, and the margins {peak, minScore, order}: the closest comparison of each kind."""
    ny, nx = S.shape
    flat = S.reshape(-1)
    peaks, m_peak = [], np.inf
    for c in np.flatnonzero(flat >= min_score):
        iy, ix = divmod(int(c), nx)
        ok = True
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                jx, jy = ix + dx, iy + dy
                if (dx == 0 and dy == 0) or not (0 <= jx < nx and 0 <= jy < ny):
                    continue
                v = S[jy, jx]
                m_peak = min(m_peak, float(abs(flat[c] - v)))
                ok = ok and (flat[c] > v if jy * nx + jx < c else flat[c] >= v)
        if ok:
            peaks.append(int(c))
    peaks.sort(key=lambda c: (-flat[c], c))
    sc_ = [flat[c] for c in peaks]
    m_order = min([float(a - b) for a, b in zip(sc_[:max_cand], sc_[1:max_cand + 1])], default=np.inf)   # the kept ones, and the last kept against the first dropped
    return peaks[:max_cand], sc_[:max_cand], dict(peak=m_peak, minScore=float(np.abs(flat - LD(min_score)).min()), order=m_order)


def _solve2(h11, h12, h22, b1, b2):
    det = h11 * h22 - h12 * h12
    return (h22 * b1 - h12 * b2) / det, (h11 * b2 - h12 * b1) / det, det


def localize(sc, S, minScore=None, maxCand=64, minLinks=3, gate=4.0, iters=8, maxMove=None, maxTargets=64):
    """Stages B and C on the map S [ny x nx] (anything NumPy; compared as it is).  Returns a namespace: pos, vel, vel_status, score, n_links, assoc (in the GIVEN order
    of the measurements), rms per target; cand_cell, cand_score, cand_status; margins (the closest comparison of each kind); pos_bound, vel_bound, rms_bound per target
    (for eps = the scene's per-residual rounding, map_bound(sc)[1])."""
    x0, dx, nx, y0, dy, ny = sc.grid
    minScore = minLinks - 0.5 if minScore is None else minScore
    maxMove = 4.0 * float(np.hypot(dx, dy)) if maxMove is None else maxMove
    eps = map_bound(sc)[1]
    cells, scores, mg = candidates(np.asarray(S), minScore, maxCand)
    mg.update(best=np.inf, gate=np.inf, det=np.inf, maxMove=np.inf)
    K, M = len(sc.links), len(sc.link)
    claimed = np.zeros(M, dtype=bool)
    xs, ys = grid_xy(sc)
    T = SimpleNamespace(pos=[], vel=[], vel_status=[], score=[], n_links=[], assoc=[], rms=[], pos_bound=[], vel_bound=[], rms_bound=[])
    status = []
    for c, s_c in zip(cells, scores):
        iy, ix = divmod(c, nx)
        xc, yc = xs[ix], ys[iy]
        assoc = np.full(K, -1)
        for k in range(K):
            ms = [m for m in np.flatnonzero(sc.link == k) if not claimed[m]]
            if not ms:
                continue
            q = np.array([q_of(sc, m, xc, yc) for m in ms], dtype=LD)
            j = int(np.argmin(q))                                           # the lowest index on a tie
            if len(ms) > 1:
                mg["best"] = min(mg["best"], float(np.sort(q)[1] - q[j]))
            mg["gate"] = min(mg["gate"], float(abs(q[j] - LD(gate) ** 2)))
            if q[j] <= LD(gate) ** 2:
                assoc[k] = ms[j]
        used = [int(m) for m in assoc if m >= 0]
        if len(used) < minLinks:
            status.append(1)
            continue
        x, y, st, H = xc, yc, 0, None

        def normal(x, y):
            h11 = h12 = h22 = b1 = b2 = LD(0)
            jsum = jmax = 0.0
            for m in used:
                rho, alpha, gr, ga = geom(sc, m, x, y)
                for res, gx, gy in ((rho / LD(sc.sigma_r[m]), gr[0] / LD(sc.sigma_r[m]), gr[1] / LD(sc.sigma_r[m])),
                                    (alpha / LD(sc.sigma_a[m]), ga[0] / LD(sc.sigma_a[m]), ga[1] / LD(sc.sigma_a[m]))):
                    h11, h12, h22, b1, b2 = h11 + gx * gx, h12 + gx * gy, h22 + gy * gy, b1 + gx * res, b2 + gy * res
                    jsum, jmax = jsum + float(np.hypot(gx, gy)), max(jmax, float(np.hypot(gx, gy)))
            return h11, h12, h22, b1, b2, jsum, jmax
        for _ in range(iters):
            h11, h12, h22, b1, b2, _, _ = normal(x, y)
            det, thr = h11 * h22 - h12 * h12, SINGULAR * ((h11 + h22) / 2) ** 2
            mg["det"] = min(mg["det"], float(abs(det / thr - 1)) if thr > 0 else np.inf)
            if not det > thr:
                st = 2
                break
            sx, sy, _ = _solve2(h11, h12, h22, b1, b2)
            x, y = x - sx, y - sy
        if st == 0:
            move = np.sqrt((x - xc) ** 2 + (y - yc) ** 2)
            mg["maxMove"] = min(mg["maxMove"], float(abs(move - LD(maxMove))))
            if not move <= maxMove:
                st = 3
        if st == 0 and len(T.pos) >= maxTargets:
            st = 4
        status.append(st)
        if st != 0:
            continue
        h11, h12, h22, _, _, jsum, jmax = normal(x, y)
        lam_min = float((h11 + h22) / 2 - np.sqrt(((h11 - h22) / 2) ** 2 + h12 ** 2))
        pos_bound = 4.0 * jsum * eps / lam_min                              # H^-1 J^T d(res), d(res) <= eps a row; 4: the steps before the last carry theirs on
        qs = sum(q_of(sc, m, x, y) for m in used)
        n11 = n12 = n22 = r1 = r2 = LD(0)
        cnt, asum, d_min = 0, 0.0, np.inf
        for m in used:
            tx, rx = (sc.nodes[n] for n in sc.links[sc.link[m]])
            d_min = min(d_min, float(np.sqrt((x - tx[0]) ** 2 + (y - tx[1]) ** 2 + (sc.height - tx[2]) ** 2)), float(np.sqrt((x - rx[0]) ** 2 + (y - rx[1]) ** 2 + (sc.height - rx[2]) ** 2)))
            if np.isnan(sc.s[m]):
                continue
            _, _, gr, _ = geom(sc, m, x, y)
            ax, ay, ysm = -gr[0] / LD(sc.sigma_v[m]), -gr[1] / LD(sc.sigma_v[m]), LD(sc.s[m]) / LD(sc.sigma_v[m])
            n11, n12, n22, r1, r2 = n11 + ax * ax, n12 + ax * ay, n22 + ay * ay, r1 + ax * ysm, r2 + ay * ysm
            cnt, asum = cnt + 1, asum + float(np.hypot(ax, ay)) * (abs(float(ysm)) + 1.0)
        h, dl = (n11 + n22) / 2, np.sqrt(((n11 - n22) / 2) ** 2 + n12 ** 2)
        with np.errstate(invalid="ignore", divide="ignore"):
            ok = cnt >= 2 and bool((h - dl) / (h + dl) >= VEL_COND)
        if ok:
            vx, vy, _ = _solve2(n11, n12, n22, r1, r2)
            # the rows move with the position (by pos_bound / d_min of their length) and round (16 u): both through N^-1
            vel_bound = 4.0 * asum * (2.0 * pos_bound / d_min + 16 * U) * (1.0 + float(np.hypot(vx, vy))) / float(h - dl)
        else:
            vx = vy = LD(np.nan)
            vel_bound = 0.0
        T.pos.append((x, y)); T.vel.append((vx, vy)); T.vel_status.append(0 if ok else 1); T.score.append(s_c); T.n_links.append(len(used))
        T.assoc.append([int(sc.order[m]) if m >= 0 else -1 for m in assoc]); T.rms.append(np.sqrt(qs / len(used)))
        T.pos_bound.append(pos_bound); T.vel_bound.append(vel_bound); T.rms_bound.append(eps + jmax * pos_bound + 8 * U * float(np.sqrt(qs / len(used))))
        claimed[used] = True
    return SimpleNamespace(pos=np.array(T.pos, dtype=LD).reshape(-1, 2), vel=np.array(T.vel, dtype=LD).reshape(-1, 2), vel_status=np.array(T.vel_status, dtype=np.int32),
                           score=np.array(T.score, dtype=LD), n_links=np.array(T.n_links, dtype=np.int32), assoc=np.array(T.assoc, dtype=np.int32).reshape(-1, K),
                           rms=np.array(T.rms, dtype=LD), pos_bound=np.array(T.pos_bound), vel_bound=np.array(T.vel_bound), rms_bound=np.array(T.rms_bound),
                           cand_cell=np.array(cells, dtype=np.int32), cand_score=np.array(scores, dtype=LD), cand_status=np.array(status, dtype=np.int32), margins=mg)


# ---------------------------------------------------------------- exact measurements of targets
def exact_meas(nodes, links, targets, velocities=None, azimuth=True, sigma=(2.0, 1.0, 2.0), err=None, rng=None):
    """One measurement per (link, target): r, s and azi of `targets` [Q x 3] moving with `velocities` [Q x 3], link by link; `err` = (metres, degrees): uniform errors of
    that half-width on r and azi."""
    nodes, targets = np.asarray(nodes, dtype=np.float64), np.asarray(targets, dtype=np.float64)
    velocities = np.zeros_like(targets) if velocities is None else np.asarray(velocities, dtype=np.float64)
    out = {k: [] for k in ("link", "r", "s", "azi")}
    for k, (t, r) in enumerate(links):
        for p, v in zip(targets, velocities):
            dt, dr = p - nodes[t], p - nodes[r]
            out["link"].append(k)
            out["r"].append(np.sqrt(dt @ dt) + np.sqrt(dr @ dr) + (rng.uniform(-err[0], err[0]) if err else 0.0))
            out["s"].append(-(v @ dt) / np.sqrt(dt @ dt) - (v @ dr) / np.sqrt(dr @ dr))
            out["azi"].append(np.rad2deg(np.arctan2(dr[1], dr[0])) + (rng.uniform(-err[1], err[1]) if err else 0.0) if azimuth else np.nan)
    n = len(out["link"])
    return dict(link=np.array(out["link"], dtype=np.int32), r=np.array(out["r"]), s=np.array(out["s"]), azi=np.array(out["azi"]), sigma_r=np.full(n, sigma[0]),
                sigma_v=np.full(n, sigma[1]), sigma_a=np.full(n, sigma[2]))


NODES3 = np.array([[0.0, 0.0, 25.0], [800.0, 0.0, 25.0], [400.0, 640.0, 30.0]])
TARGETS4 = np.array([[210.5, 310.25, 1.5], [523.75, 188.5, 1.5], [390.25, 455.0, 1.5], [655.5, 402.75, 1.5]])
VEL4 = np.array([[10.0, -3.0, 0.0], [-7.0, 12.0, 0.0], [0.0, 15.0, 0.0], [-20.0, -5.0, 0.0]])
GRID401 = (0.0, 2.0, 401, 0.0, 2.0, 401)


def all_links(n):
    return [(t, r) for t in range(n) for r in range(n)]


def prototype_scene(name, err=(0.5, 0.5), seed=11, grid=GRID401):
    """'three_nodes': three nodes, nine links, range only.  'two_nodes': two nodes, four links, with azimuth.  Four targets, errors uniform +-0.5 m and +-0.5 degrees."""
    nodes = NODES3 if name == "three_nodes" else NODES3[:2]
    links = all_links(len(nodes))
    meas = exact_meas(nodes, links, TARGETS4, VEL4, azimuth=name == "two_nodes", err=err, rng=np.random.default_rng(seed))
    return make_scene(nodes, links, meas, grid, 1.5)


def _random_scene(seed, N, K, M, grid, azimuth, sigma_r=4.0, extra=None):
    """N nodes on dyadic positions, K links, M measurements of random (sorted at random, so the stable sort is exercised) targets inside the grid."""
    rng = np.random.default_rng(seed)
    x0, dx, nx, y0, dy, ny = grid
    w, h = max(dx * (nx - 1), 8.0), max(dy * (ny - 1), 8.0)
    nodes = np.column_stack([x0 + np.round(rng.uniform(-0.5, 1.5, N) * w * 4) / 4, y0 + np.round(rng.uniform(-0.5, 1.5, N) * h * 4) / 4, np.round(rng.uniform(10, 30, N))])
    links = [(int(rng.integers(N)), int(rng.integers(N))) for _ in range(K)]
    link = rng.integers(K, size=M).astype(np.int32)
    if M >= K:
        link[:K] = rng.permutation(K)                                       # every link has one
    p = np.column_stack([x0 + rng.uniform(0, 1, M) * w, y0 + rng.uniform(0, 1, M) * h, np.full(M, 1.5)])
    r = np.array([np.linalg.norm(p[m] - nodes[links[link[m]][0]]) + np.linalg.norm(p[m] - nodes[links[link[m]][1]]) for m in range(M)]) + rng.uniform(-1, 1, M)
    azi = np.array([np.rad2deg(np.arctan2(*(p[m] - nodes[links[link[m]][1]])[1::-1])) for m in range(M)]) + rng.uniform(-1, 1, M)
    if azimuth == "none":
        azi[:] = np.nan
    elif azimuth == "mixed":
        azi[rng.uniform(size=M) < 0.5] = np.nan
    meas = dict(link=link, r=r, s=rng.uniform(-30, 30, M), azi=azi, sigma_r=np.full(M, sigma_r) * rng.choice([1.0, 1.5], M), sigma_v=np.ones(M), sigma_a=np.full(M, 3.0))
    if extra:
        extra(nodes, links, meas)
    return make_scene(nodes, links, meas, grid, 1.5)


def _underflow(nodes, links, meas):                                        # measurement 0: a range sum no grid point comes near, w = 0 everywhere
    meas["r"][0] = 1.0e4


def _near_the_point(nodes, links, meas):                                  # the 1 x 1 grid: the measurement passes 1.5 m and 1 degree from its one point
    d = np.array([64.0, 32.0, 1.5]) - nodes[0]
    meas["r"][0], meas["azi"][0] = 2.0 * np.sqrt(d @ d) + 1.5, np.rad2deg(np.arctan2(d[1], d[0])) + 1.0


def _node_on_grid(nodes, links, meas):                                     # node 0 exactly on grid point (3, 2) of the 67 x 129 grid, at the grid's height
    nodes[0] = (16.0 + 3 * 2.0, -8.0 + 2 * 0.5, 1.5)


# name -> (seed, N, K, M, grid, azimuth, extra): every grid, M, K, N and azimuth mix the GPU test names
MAP_SCENES = {
    "g1x1_m1_k1_n1": (1, 1, 1, 1, (64.0, 2.0, 1, 32.0, 2.0, 1), "all", _near_the_point),
    "g5x3_m2_k1_n3": (2, 3, 1, 2, (0.0, 4.0, 5, 0.0, 4.0, 3), "none", None),
    "g5x3_m4096_k9_n3": (3, 3, 9, 4096, (0.0, 4.0, 5, 0.0, 4.0, 3), "mixed", None),
    "g67x129_m17_k9_n3": (4, 3, 9, 17, (16.0, 2.0, 67, -8.0, 0.5, 129), "mixed", _node_on_grid),
    "g67x129_m65_k9_n64": (5, 64, 9, 65, (16.0, 2.0, 67, -8.0, 0.5, 129), "all", _underflow),
    "g256x256_m65_k9_n3": (6, 3, 9, 65, (0.0, 2.0, 256, 0.0, 2.0, 256), "none", None),
    "g67x129_m300_k256_n64": (7, 64, 256, 300, (16.0, 2.0, 67, -8.0, 0.5, 129), "mixed", None),
}


@lru_cache(maxsize=None)
def map_scene(name):
    seed, N, K, M, grid, azimuth, extra = MAP_SCENES[name]
    sc = _random_scene(seed, N, K, M, grid, azimuth, sigma_r=8.0 if K == 256 else 4.0, extra=extra)
    sc.ref_map = position_map(sc)
    sc.bound = map_bound(sc)[0]
    return sc


# the full-chain scenes: name -> (prototype, parameters, what is done to the measurements)
def _one_doppler(meas):                                                    # a single finite s per target: velocity NaN
    meas["s"][meas["link"] != 0] = np.nan


CHAIN_SCENES = {
    "three_nodes": ("three_nodes", {}, None),
    "two_nodes": ("two_nodes", dict(minLinks=3), None),
    "status_1": ("three_nodes", dict(minLinks=10, minScore=8.5), None),      # nine links cannot give ten
    "status_2": ("two_nodes_line", dict(minLinks=1, minScore=0.5), None),    # one mono-static link, range only: H has rank one
    "status_3": ("three_nodes", dict(maxMove=0.25), None),                   # a quarter of a metre: the errors move the fix further
    "one_doppler": ("three_nodes", {}, _one_doppler),
}


@lru_cache(maxsize=None)
def chain_scene(name):
    proto, par, change = CHAIN_SCENES[name]
    if proto == "two_nodes_line":
        node = np.array([[3.2578125, -7.640625, 25.0]])                                # off the integers: no two grid points at one distance
        meas = exact_meas(node, [(0, 0)], TARGETS4[:1], VEL4[:1], azimuth=False)
        sc = make_scene(node, [(0, 0)], meas, (100.0, 2.0, 129, 200.0, 2.0, 129), 1.5)
    else:
        sc = prototype_scene(proto)
        if change:
            meas = {k: np.array(v) for k, v in sc.given.items()}
            change(meas)
            sc = make_scene(sc.nodes, sc.links, meas, sc.grid, sc.height)
    sc.par = {**DEFAULTS, **par}
    sc.ref_map = position_map(sc)
    sc.bound = map_bound(sc)[0]
    sc.ref = localize(sc, sc.ref_map, **sc.par)
    return sc
