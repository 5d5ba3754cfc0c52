"""sensing.estimation.localizeTargets: the lists of several (transmitter, receiver) links fused into one position and one velocity vector per target, in the network frame
(project-defined; include/isac_localize.h: isac_position_map_dev, isac_localize_dev)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _lib as L

MEAS_FIELDS = ("link", "r", "s", "azi", "sigma_r", "sigma_v", "sigma_a")


class Scene:
    """The scene arguments both calls share, from (nodes [N x 3], links [K x 2] (tx node, rx node), meas, grid, height); keeps every host buffer alive.  ``meas``: a dict
    of ``link, r, s, azi, sigma_r, sigma_v, sigma_a`` [M] in any order of links; the calls want them sorted by link, so they are sorted stably here and ``order`` maps a
    sorted position back to the caller's index.  ``grid`` = (x0, dx, nx, y0, dy, ny)."""

    def __init__(self, nodes, links, meas, grid, height):
        self.nodes = np.ascontiguousarray(np.asarray(nodes, dtype=np.float64).reshape(-1, 3))
        lk = np.asarray(links, dtype=np.int32).reshape(-1, 2)
        self.link_tx, self.link_rx = np.ascontiguousarray(lk[:, 0]), np.ascontiguousarray(lk[:, 1])
        link = np.asarray(meas["link"], dtype=np.int32).reshape(-1)
        self.order = np.argsort(link, kind="stable")
        self.link = np.ascontiguousarray(link[self.order])
        self.f = [np.ascontiguousarray(L.as_f64(meas[k])[self.order]) for k in MEAS_FIELDS[1:]]
        if any(a.size != link.size for a in self.f):
            raise ValueError("meas: link, r, s, azi, sigma_r, sigma_v and sigma_a must have one value per measurement")
        x0, dx, nx, y0, dy, ny = grid
        self.nx, self.ny, self.K = int(nx), int(ny), int(lk.shape[0])
        self.grid = (float(x0), float(dx), self.nx, float(y0), float(dy), self.ny, float(height))

    def args(self, ctx, d_map):
        p = lambda a: a.ctypes.data_as(C.c_void_p)                           # noqa: E731
        return (ctx.handle, p(self.nodes), self.nodes.shape[0], p(self.link_tx), p(self.link_rx), self.K, p(self.link), *[p(a) for a in self.f], int(self.link.size),
                *self.grid, d_map)


def position_map(ctx, scene):
    """isac_position_map_dev: the map of ``scene`` as a DeviceArray [nx x ny] column-major, which is the call's [ny x nx] with x fastest (``.numpy().T`` is [ny x nx])."""
    if not (0 < scene.nx <= 8192 and 0 < scene.ny <= 8192):
        raise L.IsacError(1, "localizeTargets: 1 <= nx, ny <= 8192 is required")
    d_map = ctx.empty((scene.nx, scene.ny), np.float64)
    ctx.check(ctx.lib.isac_position_map_dev(*scene.args(ctx, d_map)))
    return d_map


def localize_raw(ctx, scene, d_map, minScore, maxCand, minLinks, gate, iters, maxMove, maxTargets, fill=(0.0, 0)):
    """isac_localize_dev itself: (status, the output arrays whole, as a dict).  ``fill``: what the double and the integer arrays hold before the call."""
    T, Cn, K = max(int(maxTargets), 1), max(int(maxCand), 1), scene.K
    f64 = lambda *shape: np.full(shape, fill[0], dtype=np.float64)           # noqa: E731
    i32 = lambda *shape: np.full(shape, fill[1], dtype=np.int32)             # noqa: E731
    o = dict(pos=f64(T, 2), vel=f64(T, 2), vel_status=i32(T), score=f64(T), n_links=i32(T), assoc=i32(T, K), rms=f64(T), cand_cell=i32(Cn), cand_score=f64(Cn),
             cand_status=i32(Cn), n_out=i32(2))
    st = ctx.lib.isac_localize_dev(*scene.args(ctx, d_map), float(minScore), int(maxCand), int(minLinks), float(gate), int(iters), float(maxMove), int(maxTargets),
                                   *[a.ctypes.data_as(C.c_void_p) for a in o.values()])
    return st, o


def localize(ctx, scene, d_map, minScore, maxCand, minLinks, gate, iters, maxMove, maxTargets):
    """Stages B and C on any device map [nx x ny] column-major: (targets dict, candidates dict), cut to the counts; ``assoc`` in the caller's measurement order."""
    st, o = localize_raw(ctx, scene, d_map, minScore, maxCand, minLinks, gate, iters, maxMove, maxTargets)
    ctx.check(st)
    n, nc = int(o["n_out"][0]), int(o["n_out"][1])
    tg = {k: o[k][:n].copy() for k in ("pos", "vel", "vel_status", "score", "n_links", "assoc", "rms")}
    a = tg["assoc"]
    a[a >= 0] = scene.order[a[a >= 0]]
    return tg, {k: o[k][:nc].copy() for k in ("cand_cell", "cand_score", "cand_status")}


def localizeTargets(nodes, links, meas, grid, height=0.0, minScore=None, maxCand=64, minLinks=3, gate=4.0, iters=8, maxMove=None, maxTargets=64, return_map=False,
                    return_candidates=False, ctx=None):
    """Positions and velocities of the targets that the measurements of several links agree on.

    ``nodes`` [N x 3]: the positions of the cells, metres, in the frame of gNBPosition.  ``links`` [K x 2]: (tx node, rx node) per link; tx == rx is a mono-static link.
    ``meas``: the record of sensing.estimation.linkMeasurements (``link, r, s, azi, sigma_r, sigma_v, sigma_a`` [M]: range sum R_tx + R_rx in metres; Doppler sum
    v_tx + v_rx in m/s, approaching positive, NaN = none; azimuth in degrees seen from the rx node, NaN = not used).  ``grid`` = (x0, dx, nx, y0, dy, ny): the search
    grid x0 + ix dx, y0 + iy dy on the plane of ``height``; its step should be at most about sigma_r, or the map misses peaks.

    A likelihood map over the grid counts the links that agree on each point; its local maxima of at least ``minScore`` (default minLinks - 0.5), best first and at most
    ``maxCand``, are taken one after the other: every link offers its best unclaimed measurement within ``gate`` sigmas, a candidate with fewer than ``minLinks`` links
    is dropped (that is what removes ghosts: a ghost is made of measurements real targets have claimed), ``iters`` Gauss-Newton steps refine (x, y), a point that moved
    more than ``maxMove`` metres (default: four grid diagonals) is dropped, and an accepted target claims its measurements.

    Returns a dict: ``pos`` [n x 2], ``vel`` [n x 2] (NaN where ``vel_status`` is 1: fewer than two Doppler sums, or all along one line), ``vel_status``, ``score``,
    ``n_links``, ``assoc`` [n x K] (the index into ``meas`` per link, or -1), ``rms``; with ``return_map`` also ``map`` [ny x nx]; with ``return_candidates`` also
    ``cand_cell`` (iy nx + ix), ``cand_score``, ``cand_status`` (0 accepted, 1 too few links, 2 singular, 3 moved too far, 4 table full).  Limits: include/isac_localize.h."""
    ctx = ctx or L.default_context()
    scene = Scene(nodes, links, meas, grid, height)
    if minScore is None:
        minScore = minLinks - 0.5
    if maxMove is None:
        maxMove = 4.0 * float(np.hypot(scene.grid[1], scene.grid[4]))
    d_map = position_map(ctx, scene)
    try:
        tg, cd = localize(ctx, scene, d_map, minScore, maxCand, minLinks, gate, iters, maxMove, maxTargets)
        if return_map:
            tg["map"] = np.ascontiguousarray(d_map.numpy().T)
    finally:
        d_map.free()
    if return_candidates:
        tg.update(cd)
    return tg
