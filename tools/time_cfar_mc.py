"""Trial rate of isac_cfar_monte_carlo (sensing.detection.cfarMonteCarlo): isac_timer_start / isac_timer_stop_ms (the library's event pair on the context's stream) around a
whole 2^30-trial counts-only call at the false-alarm point -- a memset, four launches of 2^28 trials, the count copy -- for CA and OS rank 18 at N = 24 and CA at N = 128,
'Auto' factor at Pfa 1e-5; 5 repetitions after a 2^26-trial warm-up each.  Beside them, for scale only, the NumPy restatement (tests/_cfar_mc_restatement.py) on the host at
2^18 trials: the figures of DESIGN.md sections 3 and 5.  Needs an MI355X:  python tools/time_cfar_mc.py"""
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from conftest import load_pkg
import _cfar_mc_restatement as MC
pkg = load_pkg()
mc = pkg.sensing.detection.cfarMonteCarlo
c = pkg.Context()
N_TRIALS = 1 << 30
for name, n, rank in (("CA", 24, 1), ("OS", 24, 18), ("CA", 128, 1)):
    mc(n, [-np.inf], 1 << 26, Method=name, Rank=rank, Pfa=1e-5, ctx=c)
    t = []
    for i in range(5):
        c.sync(); c.timer_start()
        r = mc(n, [-np.inf], N_TRIALS, Method=name, Rank=rank, Pfa=1e-5, seed=i, ctx=c)
        t.append(c.timer_stop_ms())
    print(f"{name}{' rank 18' if name == 'OS' else ''} N = {n}: 2^30 trials, event-pair ms median {np.median(t):.1f} (min {min(t):.1f}, max {max(t):.1f}) = "
          f"{N_TRIALS / np.median(t) / 1e6:.2f} G trials/s; last count {int(r.nDet[0])}", flush=True)
    n_host = 1 << 18
    alpha = r.alpha
    t0 = time.perf_counter()
    f, _ = MC.detect(MC.draw(n, 0, n_host), name, rank, alpha, "swerling0", [-np.inf])
    dt = time.perf_counter() - t0
    print(f"    NumPy restatement on the host: 2^18 trials in {dt:.2f} s = {n_host / dt / 1e6:.3f} M trials/s", flush=True)
c.close()
