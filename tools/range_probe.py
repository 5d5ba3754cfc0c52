#!/usr/bin/env python3
"""Development probe: isac_range_refine_dev (include/isac_subsample.h) at the bench shape (K 3276, L 224, A 64) beside isac_fft2d_range_stage_dev on the same grids in the
same process -- both read the two grids once per pass.  GPU times with HIP events on the context's stream (isac_timer_*), whole calls:
  probe_only  = the chunk's Doppler table + the contraction + ONE evaluation of the search kernel per entry (+ the small copies): the contraction's time to within that
  full        = the same + 17 probes and 40 halvings; full - probe_only = 57 evaluations of the search kernel for an entry that finds a maximum (its status is read and
                printed: an entry without one stops after the probes), the entries of a chunk side by side on the compute units
  python tools/range_probe.py [--ants 64] [--reps 10]"""
import argparse, ctypes as C, importlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench

ap = argparse.ArgumentParser(); ap.add_argument("--ants", type=int, default=64); ap.add_argument("--reps", type=int, default=10)
args = ap.parse_args()
pkg = importlib.import_module(bench.PKG)
cell = bench.Cell(pkg, 0, 0, args.ants, 16, 1)
ctx = cell.ctx; lib = ctx.lib; echo = cell.echo[0]
for _ in range(2):
    cell.step()
_m = importlib.import_module(bench.PKG + ".sensing.estimation.fft2D"); _mm = importlib.import_module(bench.PKG + ".sensing._marshal")
rr = importlib.import_module(bench.PKG + ".sensing.estimation.refineRange").range_refine
cf, ep = _m._cfar_block(cell.cfar), _mm.est_block(cell.rp)
K, L, A = cell.K, cell.Lsym, cell.A
gb = 2 * K * L * A * 16 / 1e9

def timed(fn):
    ts = []
    for _ in range(args.reps):
        ctx.sync(); ctx.timer_start(); fn(); ts.append(ctx.timer_stop_ms())
    return min(ts), float(np.median(ts))

def range_stage(): ctx.check(lib.isac_fft2d_range_stage_dev(ctx.handle, C.byref(ep), C.byref(cf), echo, cell.tx_grid, K, L, A))
range_stage()
mn0, med0 = timed(range_stage)
print(f"K {K} L {L} A {A}: the two grids {gb:.3f} GB")
print(f"range stage                       min {mn0:8.3f} ms  median {med0:8.3f} ms  ({gb / mn0 * 1e3:6.0f} GB/s of grid reads)")
rng = np.random.default_rng(1)
for n in (1, 16, 64):
    row = rng.integers(50, 400, n).astype(np.int32); nu = rng.uniform(-0.4, 0.4, n)
    rr(ctx, echo, cell.tx_grid, cell.rp, row, nu, probeOnly=True)
    mp, medp = timed(lambda: rr(ctx, echo, cell.tx_grid, cell.rp, row, nu, probeOnly=True))
    mf, medf = timed(lambda: rr(ctx, echo, cell.tx_grid, cell.rp, row, nu))
    passes = -(-n // 16)
    ctx.check(lib.isac_profile_enable(ctx.handle, 1))                      # the event pair around the contraction launch of the last chunk
    ks = []
    for _ in range(args.reps):
        rr(ctx, echo, cell.tx_grid, cell.rp, row, nu, probeOnly=True)
        ms = C.c_double(0); ctx.check(lib.isac_profile_last_kernel_ms(ctx.handle, C.byref(ms))); ks.append(ms.value)
    ctx.check(lib.isac_profile_enable(ctx.handle, 0))
    print(f"range refine n {n:3d} contraction     min {min(ks):8.3f} ms  median {float(np.median(ks)):8.3f} ms  (one launch: {gb / min(ks) * 1e3:6.0f} GB/s, {min(ks) / mn0:5.2f} x the range stage)")
    print(f"range refine n {n:3d} probe_only      min {mp:8.3f} ms  median {medp:8.3f} ms  ({passes} pass(es): {mp / passes:7.3f} ms each, {gb * passes / mp * 1e3:6.0f} GB/s, {mp / passes / mn0:5.2f} x the range stage)")
    # what the search ran: an entry with status 0 makes 17 + 40 + 1 = 58 evaluations (57 more than probe_only's one), one with status 1 (no maximum within a bin of its
    # row) 17 + 1; a chunk's entries run side by side, so a chunk takes as long as its longest entry
    status = rr(ctx, echo, cell.tx_grid, cell.rp, row, nu)[0]
    extra = [57 if (status[i:i + 16] == 0).any() else 17 for i in range(0, n, 16)]
    print(f"range refine n {n:3d} full            min {mf:8.3f} ms  median {medf:8.3f} ms  (status 0: {int((status == 0).sum())} of {n}, in {sum(e == 57 for e in extra)} of {passes} chunk(s); "
          f"search: {mf - mp:7.3f} ms for {sum(extra)} evaluations one after another: {(mf - mp) / sum(extra) * 1e3:6.1f} us each, {(mf - mp) / passes:7.3f} ms per chunk)")
