"""Times track_step_kernel (csrc/track.hip) on the device: isac_track_step_dev with isac_profile_enable(ctx, 1), the event pair around the launch
(isac_profile_last_kernel_ms).  Shapes: B = 256 and B = 1024 banks of T = 64 live tracks taking 16 fixes and nine links x 16 measurements a scan, and the single-bank worst
case T = 256 with 256 fixes in one group.  Seven launches each; the first launch of the process is reported apart.  Run from the repository root:  python tools/time_track.py"""
from __future__ import annotations

import ctypes as C
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("5g_based_system_level_integrated_sensing_and_communication_simulator_amd")

NODES = np.array([[0.0, 0.0, 25.0], [800.0, 0.0, 25.0], [400.0, 700.0, 30.0]])
LINKS = np.array([(t, r) for r in range(3) for t in range(3)], dtype=np.int32)
HEIGHT = 1.5


def link_values(p, v, k):
    """Range sum and Doppler sum of the points p [.. x 2] moving with v on link k."""
    q = np.concatenate([p, np.full(p.shape[:-1] + (1,), HEIGHT)], axis=-1)
    a, b = q - NODES[LINKS[k, 0]], q - NODES[LINKS[k, 1]]
    da, db = np.linalg.norm(a, axis=-1), np.linalg.norm(b, axis=-1)
    g = a[..., :2] / da[..., None] + b[..., :2] / db[..., None]
    return da + db, -(v * g).sum(axis=-1)


def bank_records(rng, B, Q, p, v, scan, first):
    """Per bank: the birth scan (Q fixes) or a timed scan (16 fixes of group 0, then 16 measurements on each of the nine links, groups 1 .. 9)."""
    recs = []
    for b in range(B):
        if first:
            z = np.column_stack([p[b] + rng.normal(0, 1.0, (Q, 2)), v[b] + rng.normal(0, 0.5, (Q, 2))])
            recs.append(dict(group=np.zeros(Q, dtype=np.int32), kind=np.zeros(Q, dtype=np.int32), link=np.zeros(Q, dtype=np.int32), z=z, sigma=np.tile([1.0, 1.0, 0.5, 0.5], (Q, 1))))
            continue
        pick = (np.arange(16) * 4 + scan) % Q
        group, kind, link = [np.zeros(16, dtype=np.int32)], [np.zeros(16, dtype=np.int32)], [np.zeros(16, dtype=np.int32)]
        z = [np.column_stack([p[b, pick] + rng.normal(0, 1.0, (16, 2)), v[b, pick] + rng.normal(0, 0.5, (16, 2))])]
        sigma = [np.tile([1.0, 1.0, 0.5, 0.5], (16, 1))]
        for k in range(9):
            pick = (np.arange(16) * 4 + scan + k + 1) % Q
            r, s = link_values(p[b, pick], v[b, pick], k)
            group.append(np.full(16, 1 + k, dtype=np.int32)); kind.append(np.ones(16, dtype=np.int32)); link.append(np.full(16, k, dtype=np.int32))
            z.append(np.column_stack([r + rng.normal(0, 1.0, 16), np.full(16, np.nan), s + rng.normal(0, 0.5, 16), np.zeros(16)]))
            sigma.append(np.tile([1.0, 1.0, 0.5, 1.0], (16, 1)))
        recs.append(dict(group=np.concatenate(group), kind=np.concatenate(kind), link=np.concatenate(link), z=np.vstack(z), sigma=np.vstack(sigma)))
    return recs


def last_ms(ctx):
    ms = C.c_double(0.0)
    ctx.check(ctx.lib.isac_profile_last_kernel_ms(ctx.handle, C.byref(ms)))
    return ms.value


def many_banks(ctx, B, launches=7):
    rng = np.random.default_rng(B)
    Q, dt = 64, 0.4
    ix, iy = np.meshgrid(np.arange(8), np.arange(8))
    p = np.stack([100.0 + 75.0 * ix.ravel(), 80.0 + 70.0 * iy.ravel()], axis=1)[None] + rng.uniform(-10, 10, (B, Q, 2))
    v = rng.uniform(-8, 8, (B, Q, 2))
    trk = pkg.sensing.estimation.Tracker(NODES, LINKS, banks=B, maxTracks=Q, height=HEIGHT, ctx=ctx)
    try:
        o = trk.step(bank_records(rng, B, Q, p, v, 0, True), 0.0)
        birth = last_ms(ctx)
        times, live, upd = [], [], []
        for i in range(launches):
            p = p + v * dt
            o = trk.step(bank_records(rng, B, Q, p, v, i, False), dt)
            times.append(last_ms(ctx))
            live.append(int((o["status"] > 0).sum()))
            upd.append(int(sum((k == 1).sum() for k in o["assoc_kind"])))
        return birth, times, live, upd
    finally:
        trk.close()


def worst_case(ctx, launches=7):
    rng = np.random.default_rng(7)
    Q, dt = 256, 0.4
    ix, iy = np.meshgrid(np.arange(16), np.arange(16))
    p = np.stack([60.0 * ix.ravel(), 60.0 * iy.ravel()], axis=1)[None] + rng.uniform(-5, 5, (1, Q, 2))
    v = rng.uniform(-4, 4, (1, Q, 2))
    trk = pkg.sensing.estimation.Tracker(NODES, LINKS, banks=1, maxTracks=Q, height=HEIGHT, ctx=ctx)
    try:
        trk.step(bank_records(rng, 1, Q, p, v, 0, True)[0], 0.0)
        times, upd = [], []
        for i in range(launches):
            p = p + v * dt
            o = trk.step(bank_records(rng, 1, Q, p, v, 0, True)[0], dt)
            times.append(last_ms(ctx))
            upd.append(int((o["assoc_kind"] == 1).sum()))
        return times, upd
    finally:
        trk.close()


def main():
    ctx = pkg.Context()
    ctx.check(ctx.lib.isac_profile_enable(ctx.handle, 1))
    fmt = lambda ts: " ".join(f"{t:8.4f}" for t in ts)                      # noqa: E731
    print("track_step_kernel by device events (isac_profile_last_kernel_ms), milliseconds, seven launches (consecutive scans) each")
    first = None
    for B in (256, 1024):
        birth, times, live, upd = many_banks(ctx, B)
        if first is None:
            first = birth
            print(f"  the first launch of the process (B = 256, T = 64, the birth scan of 64 fixes a bank): {birth:.4f}")
        pairs = B * 64 * (16 + 9 * 16)
        med = float(np.median(times))
        print(f"  B = {B:4d}, T = 64 live, 16 fixes + 9 x 16 link measurements a bank: {fmt(times)}   min {min(times):.4f}  median {med:.4f}")
        print(f"      live tracks {live[-1]}, updates applied in the last scan {upd[-1]}; {pairs} (track, measurement) pairs a scan: {pairs / (med * 1e-3):.3e} pairs/s")
    times, upd = worst_case(ctx)
    med = float(np.median(times))
    print(f"  B = 1, T = 256 live, 256 fixes in one group: {fmt(times)}   min {min(times):.4f}  median {med:.4f}")
    print(f"      updates applied in the last scan {upd[-1]} (one greedy round each); 65536 pairs a scan: {65536 / (med * 1e-3):.3e} pairs/s, {med * 1e3 / max(upd[-1], 1):.2f} us a round")
    ctx.close()


if __name__ == "__main__":
    main()
