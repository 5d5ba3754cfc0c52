"""isac_fft2d_redetect on scene a4_273prb of tests/_target_list_restatement.py (K = 3276, L = 56, A = 4; 370 x 23 CUTs, N = 24): isac_timer_start / isac_timer_stop_ms (the
library's event pair on the context's stream) around the whole call -- memset, two launches, the count copy, one list copy per antenna with detections, the host half --
per method, 20 repetitions after 5 warm-ups: the figures of DESIGN.md section 3.  Needs an MI355X:  python tools/time_redetect.py
With --fft2d N it runs N plain fft2D calls of the same scene instead: under `rocprofv3 --kernel-trace --stats` that gives the CA panel detector's own time on the same
window (cfar_panel_kernel + cfar_merge_kernel)."""
import ctypes as C
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from conftest import load_pkg
import _target_list_restatement as R
pkg = load_pkg()
L = pkg._lib
sc = R.make("a4_273prb")
rp = pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)
cf = pkg.sensing.detection.cfar2D(rp)
c = pkg.Context()
d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
echo = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, noise=sc.noise, nfft=sc.wave.Nfft, ctx=c)
if "--fft2d" in sys.argv:
    for _ in range(int(sys.argv[sys.argv.index("--fft2d") + 1])):
        pkg.sensing.estimation.fft2D(rp, cf, echo, d_txg, ctx=c)
    c.close()
    sys.exit(0)
pkg.sensing.estimation.fft2D(rp, cf, echo, d_txg, ctx=c)
res, n_total = L.EstResult(), C.c_int32(0)
for name, rank in (("CA", 1), ("GOCA", 1), ("SOCA", 1), ("OS", 18)):
    m = L.CfarMethod(L.CFAR_METHODS[name], rank, 0.0)
    t = []
    for i in range(25):
        c.sync(); c.timer_start()
        c.check(c.lib.isac_fft2d_redetect(c.handle, C.byref(m), C.byref(res), None, None, 1 << 30, None, C.byref(n_total)))
        ms = c.timer_stop_ms()
        if i >= 5:
            t.append(ms)
    print(f"{name}{' rank 18' if name == 'OS' else ''}: {n_total.value} detections, numDets {res.num_dets}; event-pair ms median {np.median(t):.3f} (min {min(t):.3f}, max {max(t):.3f})")
c.close()
