"""isac_fft2d_get_targets at the bench shape (K = 3276, L = 224, A = 64, lazy echo grid): isac_timer_start / isac_timer_stop_ms (the library's event pair on the context's
stream) around the whole call, next to the blocking CPI of the same run -- the figure of DESIGN.md section 3.  Needs an MI355X:  python tools/time_target_list.py"""
import sys, os, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from conftest import make_scene, load_pkg
pkg = load_pkg()
sc = make_scene(n_ants=64, n_slots=16, with_noise=False, seed=3)
rp = pkg.sensing.radarParams(sc.cell, sc.carrier, sc.wave)
cf = pkg.sensing.detection.cfar2D(rp)
c = pkg.Context()
d_txg, d_wave = c.to_device(sc.tx_grid), c.to_device(sc.tx_wave)
def cpi(seed):
    lz = pkg.sensing.monoStaticSensing(d_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, nfft=4096, fuse_fft2d=(rp, cf, d_txg), ctx=c, lazy=True, seed=seed, noise_domain="spectral")
    return pkg.sensing.estimation.fft2D(rp, cf, lz, d_txg, reuse_range=True, ctx=c)
for i in range(5):
    cpi(i); pkg.sensing.estimation.targetList(c)
t_cpi, t_tl, n = [], [], 0
for i in range(20):
    c.sync(); c.timer_start(); cpi(100 + i); t_cpi.append(c.timer_stop_ms())
    c.timer_start(); tl = pkg.sensing.estimation.targetList(c); t_tl.append(c.timer_stop_ms()); n = tl["n_total"]
    w0 = time.perf_counter(); pkg.sensing.estimation.targetList(c); w = (time.perf_counter() - w0) * 1e3
print(f"targets {n}; blocking CPI ms median {np.median(t_cpi):.3f} (min {min(t_cpi):.3f}, max {max(t_cpi):.3f}); get_targets event-pair ms median {np.median(t_tl):.3f} "
      f"(min {min(t_tl):.3f}, max {max(t_tl):.3f}); last host wall ms {w:.3f}")
c.close()
