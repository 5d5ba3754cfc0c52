"""sensing.estimation.trackTargets: tracks across CPIs -- banks of constant-velocity Kalman tracks on the device that take position fixes and per-link measurements scan after
scan (project-defined; include/isac_track.h: isac_track_state_bytes, isac_track_reset_dev, isac_track_step_dev, isac_track_get_dev)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _lib as L

TABLE_FIELDS = (("status", np.int32, ()), ("id", np.int32, ()), ("age", np.int32, ()), ("hits", np.int32, ()), ("misses", np.int32, ()), ("x", np.float64, (4,)),
                ("P", np.float64, (4, 4)), ("nis", np.float64, ()), ("dof", np.int32, ()))
MEAS_FIELDS = ("group", "kind", "link", "z", "sigma")


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Scan:
    """The measurement arguments of one isac_track_step_dev call from one record per bank (``group, kind, link`` [M], ``z, sigma`` [M x 4] each): the call wants a bank's
    measurements sorted by group, so they are sorted stably here; ``order[b]`` maps a sorted position inside bank b back to the caller's index."""

    def __init__(self, records):
        self.order, parts = [], {k: [] for k in MEAS_FIELDS}
        first = [0]
        for rec in records:
            group = np.asarray(rec["group"], dtype=np.int32).reshape(-1)
            o = np.argsort(group, kind="stable")
            self.order.append(o)
            parts["group"].append(group[o])
            for k in ("kind", "link"):
                a = np.asarray(rec[k], dtype=np.int32).reshape(-1)
                if a.size != group.size:
                    raise ValueError("Tracker: group, kind and link must have one value per measurement, z and sigma four")
                parts[k].append(a[o])
            for k in ("z", "sigma"):
                a = np.asarray(rec[k], dtype=np.float64).reshape(-1, 4)
                if a.shape[0] != group.size:
                    raise ValueError("Tracker: group, kind and link must have one value per measurement, z and sigma four")
                parts[k].append(a[o])
            first.append(first[-1] + group.size)
        self.bank_first = np.asarray(first, dtype=np.int32)
        self.M = int(first[-1])
        self.f = [np.ascontiguousarray(np.concatenate(parts[k])) for k in MEAS_FIELDS]

    def args(self):
        return (_ptr(self.bank_first), *[_ptr(a) for a in self.f])


def table_arrays(B, T):
    """The nine arrays of the track table, [B x T] each (x [B x T x 4], P [B x T x 4 x 4])."""
    return {k: np.zeros((B, T) + shape, dtype=dt) for k, dt, shape in TABLE_FIELDS}


class Tracker:
    """``banks`` independent trackers of ``maxTracks`` slots each over one scene.

    ``nodes`` [N x 3] and ``links`` [K x 2] (tx node, rx node) as in localizeTargets; ``height``: the plane the tracks live on.  A track's state is (x, y, vx, vy) with a
    constant-velocity model driven by white acceleration of standard deviation ``sigmaAcc`` (m/s^2).  Every scan (``step``) predicts the tracks, then associates the
    measurements group by group -- greedily, the smallest distance first, within ``gate`` sigmas -- and updates with a sequential scalar EKF; a fix no track took starts a
    tentative track (velocity 0 +- ``initV0`` m/s where the fix has none).  A tentative track is confirmed at ``confirmHits`` scans with a measurement and dropped at
    ``tentMisses`` scans in a row without one; a confirmed track is dropped at ``maxMisses``.  The definition and the limits: include/isac_track.h."""

    def __init__(self, nodes, links, banks=1, maxTracks=64, height=0.0, sigmaAcc=1.0, gate=4.0, confirmHits=3, tentMisses=1, maxMisses=3, initV0=30.0, ctx=None):
        self.ctx = ctx or L.default_context()
        self.nodes = np.ascontiguousarray(np.asarray(nodes, dtype=np.float64).reshape(-1, 3))
        lk = np.asarray(links, dtype=np.int32).reshape(-1, 2)
        self.link_tx, self.link_rx = np.ascontiguousarray(lk[:, 0]), np.ascontiguousarray(lk[:, 1])
        self.B, self.T, self.height = int(banks), int(maxTracks), float(height)
        self.par = (float(sigmaAcc), float(gate), int(confirmHits), int(tentMisses), int(maxMisses), float(initV0))
        nbytes = int(self.ctx.lib.isac_track_state_bytes(self.B, self.T))
        if nbytes <= 0:
            raise L.IsacError(1, "Tracker: 1 <= banks <= 1024 and 1 <= maxTracks <= 256 are required")
        self.state = self.ctx.empty((nbytes,), np.uint8)
        self.reset()

    def reset(self):
        """Every slot free, every bank's id counter back to 0."""
        self.ctx.check(self.ctx.lib.isac_track_reset_dev(self.ctx.handle, self.state, self.B, self.T))

    def close(self):
        if self.state is not None:
            self.state.free()
            self.state = None

    def step(self, meas, dt):
        """One scan.  ``meas``: the record of sensing.estimation.trackMeasurements (``group, kind, link, z, sigma``, in any order of groups) when there is one bank, else a
        sequence of one record per bank.  ``dt``: seconds since the scan before (>= 0).  Returns the table after the scan -- ``status, id, age, hits, misses, nis, dof``
        [B x T], ``x`` [B x T x 4], ``P`` [B x T x 4 x 4] -- with ``n_confirmed`` [B] and, per bank and in the caller's measurement order, ``assoc`` (the slot, or -1) and
        ``assoc_kind`` (0 none, 1 updated a track, 2 born, 3 table full): arrays for a single record, lists of arrays otherwise."""
        single = isinstance(meas, dict)
        records = [meas] if single else list(meas)
        if len(records) != self.B:
            raise ValueError(f"Tracker.step: {len(records)} records for {self.B} banks")
        scan = Scan(records)
        o = table_arrays(self.B, self.T)
        o.update(assoc=np.zeros(scan.M, dtype=np.int32), assoc_kind=np.zeros(scan.M, dtype=np.int32), n_confirmed=np.zeros(self.B, dtype=np.int32))
        self.ctx.check(self.ctx.lib.isac_track_step_dev(self.ctx.handle, self.state, self.B, self.T, _ptr(self.nodes), self.nodes.shape[0], _ptr(self.link_tx),
                                                        _ptr(self.link_rx), int(self.link_tx.size), self.height, float(dt), *self.par, *scan.args(),
                                                        *[_ptr(a) for a in o.values()]))
        for k in ("assoc", "assoc_kind"):
            per_bank = []
            for b, order in enumerate(scan.order):
                a = np.empty(order.size, dtype=np.int32)
                a[order] = o[k][scan.bank_first[b]:scan.bank_first[b + 1]]
                per_bank.append(a)
            o[k] = per_bank[0] if single else per_bank
        return o

    def table(self):
        """isac_track_get_dev: the table as it stands (the arrays of ``step`` without the per-measurement ones)."""
        o = table_arrays(self.B, self.T)
        self.ctx.check(self.ctx.lib.isac_track_get_dev(self.ctx.handle, self.state, self.B, self.T, *[_ptr(a) for a in o.values()]))
        return o

    def tracks(self, confirmedOnly=True):
        """Per bank, a dict of the live (``confirmedOnly``: the confirmed) tracks in slot order: ``slot, id, status, age, hits, misses`` [n], ``x`` [n x 4], ``P`` [n x 4 x 4]."""
        return tracks_of(self.table(), confirmedOnly)


def tracks_of(table, confirmedOnly=True):
    out = []
    for b in range(table["status"].shape[0]):
        keep = np.flatnonzero(table["status"][b] >= (2 if confirmedOnly else 1))
        out.append(dict(slot=keep.astype(np.int32), **{k: table[k][b][keep].copy() for k in ("id", "status", "age", "hits", "misses", "x", "P")}))
    return out


def trackTargets(scans, dts, nodes, links, ctx=None, **par):
    """A sequence of scans through a fresh Tracker: ``scans[i]`` is what ``Tracker.step`` takes, ``dts[i]`` the time since the scan before.  ``par``: the Tracker's keyword
    arguments.  Returns the history: per scan a dict of ``tracks`` (per bank, the live tracks: ``Tracker.tracks(confirmedOnly=False)``), ``assoc``, ``assoc_kind`` and
    ``n_confirmed``."""
    trk = Tracker(nodes, links, ctx=ctx, **par)
    try:
        history = []
        for meas, dt in zip(scans, dts):
            o = trk.step(meas, dt)
            history.append(dict(tracks=tracks_of(o, confirmedOnly=False), assoc=o["assoc"], assoc_kind=o["assoc_kind"], n_confirmed=o["n_confirmed"]))
        return history
    finally:
        trk.close()
