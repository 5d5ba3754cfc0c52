"""Development measurement (not part of the product): isac_rx_frontend_batch_dev at config 5's two batch shapes -- uplink 10 x [61 909 x 64], downlink 40 x [61 909 x 2] --
in the modes NONE and PHILOX, HIP events around the launch (isac_timer_start / isac_timer_stop_ms), warm, median of 30; then tools/cbench's flat copy of the same number
of bytes in the same session.  Prints the text kept as profiles/rx_frontend_kernel_times.txt.
    python tools/rxfe_bench.py [out.txt]      (build tools/cbench first: see tools/cbench.hip)"""
import importlib
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module("5g_based_system_level_integrated_sensing_and_communication_simulator_amd")
L = pkg._lib
T, REPS, WARM = 61909, 30, 5
NT = 1.380649e-23 * (290.0 + 290.0 * (10.0 ** 0.7 - 1.0)) * 122.88e6


def main():
    ctx = pkg.default_context()
    lines = ["# isac_rx_frontend_batch_dev (csrc/rxfe.hip), HIP events around the launch, warm, median of %d (min) | bytes = read + written" % REPS]
    res = {}
    sizes = []
    for name, n_jobs, nr in (("uplink   10 x [61909 x 64]", 10, 64), ("downlink 40 x [61909 x 2] ", 40, 2)):
        per = T * nr
        d_all = ctx.empty((n_jobs * per,))
        ctx.check(ctx.lib.isac_memset_dev(ctx.handle, d_all, 0, d_all.nbytes))
        jobs = (L.RxFrontendJob * n_jobs)()
        for j in range(n_jobs):
            jobs[j] = L.RxFrontendJob(d_all.ptr + 16 * per * j, None, 1e-6, 2.0, NT, 1000 + j)
        nbytes = n_jobs * per * 16
        sizes.append(nbytes)
        for mode_name, mode in (("NONE", L.NOISE_NONE), ("PHILOX", L.NOISE_PHILOX)):
            ms = []
            for r in range(WARM + REPS):
                ctx.timer_start()
                ctx.check(ctx.lib.isac_rx_frontend_batch_dev(ctx.handle, jobs, n_jobs, T, nr, mode))
                t = ctx.timer_stop_ms()
                if r >= WARM:
                    ms.append(t)
            med = float(np.median(ms))
            res[(name, mode_name)] = (med, nbytes)
            lines.append(f"{name} {mode_name:6s} median {med * 1e3:9.2f} us  (min {min(ms) * 1e3:9.2f})  {2 * nbytes / 1e9 / med:6.3f} TB/s  [{nbytes} B per direction]")
        d_all.free()
    cb = os.path.join(ROOT, "tools", "cbench")
    copy = {}
    if os.path.exists(cb):
        out = subprocess.run([cb] + [str(s) for s in sizes], capture_output=True, text=True, timeout=300).stdout
        for ln in out.splitlines():
            f = ln.split()
            if f and f[0] == "flat_copy":
                copy[int(f[2])] = float(f[4]) / 1e3
                lines.append("tools/cbench " + ln)
    else:
        lines.append("tools/cbench not built: no copy yardstick in this session")
    for (name, mode_name), (med, nbytes) in res.items():
        extra = f"  x{med / copy[nbytes]:.2f} of the flat copy" if nbytes in copy else ""
        lines.append(f"ratio {name} {mode_name:6s}{extra}")
    for name in sorted({k[0] for k in res}):
        lines.append(f"ratio {name} PHILOX / NONE = {res[(name, 'PHILOX')][0] / res[(name, 'NONE')][0]:.2f}")
    # config 5's frame: 3 360 downlink + 840 uplink applies, batched 40 / 10 per launch as measured above
    for mode_name in ("NONE", "PHILOX"):
        ul = next(v for k, v in res.items() if k[0].startswith("uplink") and k[1] == mode_name)[0]
        dl = next(v for k, v in res.items() if k[0].startswith("downlink") and k[1] == mode_name)[0]
        lines.append(f"config 5 frame ({mode_name}): 84 downlink launches x {dl:.4f} ms + 84 uplink launches x {ul:.4f} ms = {84 * dl + 84 * ul:.2f} ms")
    text = "\n".join(lines) + "\n"
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        open(sys.argv[1], "w").write(text)


if __name__ == "__main__":
    main()
