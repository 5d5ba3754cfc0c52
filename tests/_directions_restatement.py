"""NumPy restatement of isac_resolve_directions (include/isac_directions.h, DESIGN.md section 5 -- project-defined): the greedy pass, the maximiser and the RELAX cycles on
array snapshots, and the synthetic scenes its tests share.  For import only.

Every sum and every maximiser runs in np.longdouble; the maximiser bisects the analytic derivative 60 times (the box is half a lobe wide: 4e-19 of a lobe, far below the
1e-12 the tests need).  One geometry serves both arrays, as in the library: element e = n + ny m at phase 2 pi d (m u + n v); the ULA is ny = 1, u = f / d, v = 0.
The order by power, n_src and the angles are formed in float64 exactly as the library's host code forms them."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

D_SPACING = 0.5
N_BISECT = 60
ROUNDS = 3
MAX_SOURCES = 8
_LD, _CLD = np.longdouble, np.clongdouble
_PI = 4 * np.arctan(_LD(1))


def geom(A, upa=None):
    """upa: None (ULA) or (n_ants_x, n_ants_y)."""
    nx, ny = (A, 1) if upa is None else upa
    assert nx * ny == A
    e = np.arange(A)
    return SimpleNamespace(A=A, nx=nx, ny=ny, Gu=4 * nx, Gv=4 * ny if upa else 1, two_d=upa is not None, m=(e // ny).astype(_LD), n=(e % ny).astype(_LD))


def lobes(g, du, dv=0.0):
    """A direction error in lobes per axis: |d dir| x (elements on that axis) x d."""
    return max(abs(float(du)) * g.nx * D_SPACING, abs(float(dv)) * g.ny * D_SPACING if g.two_d else 0.0)


def steer(g, u, v=0.0):
    """a(u, v) [A] in fp64 (for building scenes)."""
    return np.exp(-2j * np.pi * D_SPACING * (g.m.astype(np.float64) * u + g.n.astype(np.float64) * v))


def _phasor(g, u, v):
    ph = (2 * _PI * _LD(D_SPACING)) * (g.m * _LD(u) + g.n * _LD(v))
    return (np.cos(ph) + 1j * np.sin(ph)).astype(_CLD)


def _sd(g, r, u, v, axis):
    z = r * _phasor(g, u, v)
    return z.sum(), ((g.n if axis else g.m) * z).sum()


def _slope(g, r, u, v, axis):
    s, d = _sd(g, r, u, v, axis)
    return s.imag * d.real - s.real * d.imag                                # the sign carrier of dB/dt: -Im(conj(S) D)


def bartlett(g, r, u, v):
    s, _ = _sd(g, r, u, v, 0)
    return float(s.real * s.real + s.imag * s.imag)


def box_maxima(g, r, c, h, other, axis, points=65):
    """Interior local maxima of B along `axis` over a dense scan of the box [c - h, c + h]."""
    t = np.linspace(float(c) - h, float(c) + h, points)
    b = np.array([bartlett(g, r, other, x) if axis else bartlett(g, r, x, other) for x in t])
    return int(((b[1:-1] > b[:-2]) & (b[1:-1] >= b[2:])).sum())


def _axis(g, r, c, h, other, axis, log):
    f = (lambda t: _slope(g, r, other, t, 1)) if axis else (lambda t: _slope(g, r, t, other, 0))
    lo, hi = _LD(c) - _LD(h), _LD(c) + _LD(h)
    ok = f(lo) > 0 and f(hi) < 0
    if log is not None:
        log.append(box_maxima(g, r, c, h, other, axis) == 1 and bool(ok))
    if not ok:
        return _LD(c)
    for _ in range(N_BISECT):
        mid = (lo + hi) / 2
        if f(mid) > 0:
            lo = mid
        else:
            hi = mid
    return (lo + hi) / 2


def maximise(g, r, u0, v0, log=None):
    hu, hv = 2.0 / g.Gu, 2.0 / g.Gv
    u, v = _LD(u0), _LD(v0)
    if g.two_d:
        for _ in range(ROUNDS):
            u = _axis(g, r, u0, hu, v, 0, log)
            v = _axis(g, r, v0, hv, u, 1, log)
        rad = np.hypot(u, v)
        if rad > 1:
            u, v = u / rad, v / rad
    else:
        u = _axis(g, r, u0, hu, 0.0, 0, log)
        if u < -1:
            u += 2
        if u >= 1:
            u -= 2
    return u, v


def grid(g):
    gu = -1.0 + (2.0 * np.arange(g.Gu)) / g.Gu
    gv = -1.0 + (2.0 * np.arange(g.Gv)) / g.Gv if g.two_d else np.zeros(1)
    return gu, gv


def coarse(g, r):
    """(u, v) of the first arg-max over the coarse grid (index g_u + G_u g_v), or None when the maximum is 0 or NaN."""
    gu, gv = grid(g)
    two_pi_d = 2 * _PI * _LD(D_SPACING)
    mx, ny_ = np.arange(g.nx).astype(_LD), np.arange(g.ny).astype(_LD)
    pu, pv = two_pi_d * mx[:, None] * gu.astype(_LD)[None, :], two_pi_d * ny_[:, None] * gv.astype(_LD)[None, :]
    eu, ev = (np.cos(pu) + 1j * np.sin(pu)).astype(_CLD), (np.cos(pv) + 1j * np.sin(pv)).astype(_CLD)
    s = eu.T @ r.reshape(g.nx, g.ny) @ ev                                  # [Gu x Gv]
    b = (s.real * s.real + s.imag * s.imag).astype(np.float64)
    b[gu[:, None] * gu[:, None] + gv[None, :] * gv[None, :] > 1.0] = -1.0
    b = np.where(np.isnan(b), -1.0, b).T.ravel()                           # index g_u + G_u g_v
    i = int(np.argmax(b))
    if not b[i] > 0.0:
        return None
    return float(gu[i % g.Gu]), float(gv[i // g.Gu])


def resolve_one(g, x, K, cycles=16, log=None):
    """Step 1 on one snapshot: lists (u, v, alpha) in extraction order, and ||x - sum alpha a||^2 / A."""
    x = np.asarray(x).astype(_CLD)
    p, al = [], []

    def residual(skip=-1):
        r = x.copy()
        for i in range(len(p)):
            if i != skip:
                r = r - al[i] * np.conj(_phasor(g, *p[i]))
        return r

    for k in range(K):
        r = residual()
        c = coarse(g, r)
        if c is None:
            break
        pk = maximise(g, r, c[0], c[1], log)
        p.append(pk)
        al.append(_sd(g, r, pk[0], pk[1], 0)[0] / g.A)
        if k >= 1:
            for _ in range(cycles):
                for j in range(k + 1):
                    rj = residual(j)
                    p[j] = maximise(g, rj, float(p[j][0]), float(p[j][1]), log)
                    al[j] = _sd(g, rj, p[j][0], p[j][1], 0)[0] / g.A
    rf = residual()
    return p, al, float((rf.real * rf.real + rf.imag * rf.imag).sum() / g.A)


def resolve(x, upa=None, max_sources=1, cycles=16, min_ratio=0.01, min_power=0.0, check_boxes=False):
    """isac_resolve_directions on x [A x n]: the raw outputs ([K x n] / [n]) and, with check_boxes, boxes_ok: every box the maximiser met held exactly one interior local
    maximum (dense scan) between a rising and a falling end."""
    x = np.asarray(x, dtype=np.complex128)
    x = x.reshape(x.shape[0], -1)
    A, n = x.shape
    g, K = geom(A, upa), max_sources
    o = SimpleNamespace(status=np.zeros(n, dtype=np.int32), n_found=np.zeros(n, dtype=np.int32), n_src=np.zeros(n, dtype=np.int32), residual=np.zeros(n),
                        amp=np.zeros((K, n), dtype=np.complex128), boxes_ok=True, geom=g)
    for k in ("azi", "ele", "dir_u", "dir_v", "power"):
        setattr(o, k, np.full((K, n), np.nan))
    for i in range(n):
        log = [] if check_boxes else None
        p, al, o.residual[i] = resolve_one(g, x[:, i], K, cycles, log)
        o.boxes_ok = o.boxes_ok and (log is None or all(log))
        amp = np.array([complex(a) for a in al], dtype=np.complex128)
        pw = amp.real * amp.real + amp.imag * amp.imag
        order = np.argsort(-pw, kind="stable")
        nf = len(p)
        ns = 0
        while ns < nf and pw[order[ns]] >= min_ratio * pw[order[0]] and pw[order[ns]] >= min_power:
            ns += 1
        o.status[i], o.n_found[i], o.n_src[i] = int(nf == 0), nf, ns
        for k, s in enumerate(order):
            u, v = float(p[s][0]), float(p[s][1])
            o.dir_u[k, i], o.power[k, i], o.amp[k, i] = u, pw[s], amp[s]
            if g.two_d:
                o.dir_v[k, i] = v
                o.ele[k, i] = np.degrees(np.arcsin(min(1.0, np.hypot(u, v))))
                o.azi[k, i] = np.degrees(np.arctan2(v, u))
            else:
                o.azi[k, i] = np.degrees(np.arcsin(u))
    return o


# ---------------------------------------------------------------- synthetic scenes: noise-free sums of steering vectors.  Each entry is a list of (amplitude, azimuth
# [, elevation]) in degrees; amplitudes are complex and unequal so that no snapshot is symmetric (an exact tie between +f and -f would be broken by rounding).
def uv_of(upa, azi, ele=None):
    if upa is None:
        return np.sin(np.radians(azi)), 0.0
    st = np.sin(np.radians(ele))
    return st * np.cos(np.radians(azi)), st * np.sin(np.radians(azi))


_A1 = 0.8 + 0.3j
SINGLE = {
    # name: (A, upa, [one (amp, azi[, ele]) source per entry])
    "ula2": (2, None, [[(_A1, 17.3)]]),
    "ula4": (4, None, [[(_A1, -61.3)], [(1.0j, 3.4)], [(0.5 - 0.2j, 33.8)], [(2.0 + 0.1j, -12.6)], [(_A1, 80.2)]]),
    "ula16": (16, None, [[(_A1, 10.37)], [(1.0j, -47.4)], [(0.5 - 0.2j, 0.6)], [(2.0 + 0.1j, 71.7)], [(_A1, -22.67)]]),
    "ula64": (64, None, [[(_A1, -33.41)]]),
    "ula256": (256, None, [[(_A1, 0.5)], [(1.0j, -0.47)], [(0.5 - 0.2j, 1.52)], [(2.0 + 0.1j, 12.4)], [(_A1, -2.45)]]),   # between two integer degrees near boresight: the 1-degree grid misses the lobe
    "upa2x8": (16, (2, 8), [[(_A1, 25.0, 40.0)]]),
    "upa8x2": (16, (8, 2), [[(_A1, 25.0, 40.0)], [(1.0j, -70.0, 55.0)], [(0.5 - 0.2j, 110.0, 20.0)], [(2.0 + 0.1j, -160.0, 65.0)], [(_A1, 5.0, 10.0)]]),
    "upa4x4": (16, (4, 4), [[(_A1, 31.0, 75.0)], [(1.0j, 122.0, 48.0)], [(0.5 - 0.2j, -141.0, 62.0)], [(2.0 + 0.1j, -52.0, 33.0)], [(_A1, 78.0, 12.0)]]),   # all four azimuth quadrants
    "upa16x16": (256, (16, 16), [[(_A1, -37.2, 28.6)]]),
}
_W = 0.2 * np.exp(1.1j)                                                  # (power 0.04 of the strongest: clear of the default min_ratio 0.01)
MULTI = {
    # name: (A, upa, max_sources, entries).  Sources of an entry at least 1.5 lobes apart on an axis, strongest first.
    "ula16_two": (16, None, 2, [[(1.0, 10.37), (_W, 22.67)], [(_A1, -30.2), (0.4j, 5.3)], [(1.0j, 50.1), (0.5, 20.9)], [(2.0, -8.8), (1.0 + 0.5j, -41.0)],
                                [(_A1, 61.0), (0.3, -61.5)]]),
    "ula64_two": (64, None, 2, [[(1.0, 10.37), (_W, 13.4)]]),
    "ula256_two": (256, None, 2, [[(1.0, 0.5), (0.5j, 1.4)]]),
    "ula16_three": (16, None, 3, [[(1.0, 10.37), (0.6j, 35.2), (0.35 - 0.1j, -20.4)]]),
    "upa2x8_two": (16, (2, 8), 2, [[(1.0, 80.0, 50.0), (0.5j, -75.0, 45.0)]]),          # apart along v, the 8-element axis: a swapped nx / ny cannot separate them
    "upa8x2_two": (16, (8, 2), 2, [[(1.0, 10.0, 50.0), (0.5j, 165.0, 45.0)]]),          # apart along u
    "upa4x4_three": (16, (4, 4), 3, [[(1.0, 40.0, 70.0), (0.6j, -140.0, 65.0), (0.4 - 0.1j, 130.0, 45.0)]]),
    "upa16x16_two": (256, (16, 16), 2, [[(1.0, -37.2, 28.6), (_W, 20.0, 45.0)]]),
}


@functools.lru_cache(maxsize=None)
def scene(name):
    """x [A x n], the true (u, v, amp) per entry, the geometry and max_sources of a scene.  Shared: callers must not modify it."""
    A, upa, K, entries = (SINGLE[name][:2] + (1, SINGLE[name][2])) if name in SINGLE else MULTI[name]
    g = geom(A, upa)
    x = np.zeros((A, len(entries)), dtype=np.complex128, order="F")
    truth = []
    for i, srcs in enumerate(entries):
        t = []
        for s in srcs:
            u, v = uv_of(upa, *s[1:])
            x[:, i] += s[0] * steer(g, u, v)
            t.append((u, v, complex(s[0])))
        truth.append(t)
    return SimpleNamespace(name=name, A=A, upa=upa, K=K, x=x, truth=truth, geom=g, n=len(entries))


@functools.lru_cache(maxsize=None)
def reference(name, max_sources=None, cycles=16):
    """The restatement's answer for a scene, computed once and shared; callers must not modify it."""
    s = scene(name)
    return resolve(s.x, s.upa, s.K if max_sources is None else max_sources, cycles, check_boxes=True)


def truth_error(s, o, i):
    """The largest direction error in lobes of entry i's sources against the truth (same strongest-first order), and the largest relative amplitude error."""
    e_dir = e_amp = 0.0
    for k, (u, v, a) in enumerate(s.truth[i]):
        e_dir = max(e_dir, lobes(s.geom, o.dir_u[k, i] - u, (o.dir_v[k, i] - v) if s.geom.two_d else 0.0))
        e_amp = max(e_amp, abs(o.amp[k, i] - a) / abs(a))
    return e_dir, e_amp


# ---------------------------------------------------------------- end to end: two targets in ONE range-Doppler cell (same range, same velocity, azimuths 10.4 and 40.7
# degrees) and one target alone at 10.4 degrees, on the smallest grid of the target-list scenes (24 PRB, 28 symbols, nFFT 64).  16 elements for the pair: fft2D's channel
# estimate multiplies receive element m by the conjugate of the SAME element's transmit grid, so the other elements' independent QPSK streams stay in the snapshot as
# self-interference that no noise setting removes -- with 4 or 8 elements it moves the two directions by 1e-3 .. 5e-3 in sind, at or beyond the 0.1 degrees the test asks
# for; with 16 the measured errors are 1.8e-4 and 1.4e-5.
def _pos(azi, rho=60.0):
    return (rho * np.cos(np.radians(azi)), rho * np.sin(np.radians(azi)), 1.5)


_E2E = dict(n_slots=2, nrb=24, num_slots_param=6, seed=31, zero_s_slots=False)
E2E = {
    "pair": dict(n_ants=16, targets=(_pos(10.4), _pos(40.7)), velocity=(7.0, 7.0), **_E2E),
    "single": dict(n_ants=4, targets=(_pos(10.4),), velocity=(7.0,), **_E2E),
}


def make_e2e(name):
    from conftest import make_scene
    return make_scene(**E2E[name])


def apparent_u(sc):
    """dir_u of every target as its echo shows it in a snapshot of fft2D.  The coherent part of the snapshot is the SQUARE of radarParams' steering vector (once from
    the target's illumination through the element's own transmit stream, once on receive), and radarParams.m:95 divides a spacing in wavelengths by the wavelength in
    metres: with psi the phase step of that vector, x[m] ~ e^{2 j psi m} = e^{-j pi m u}, u = -2 psi / pi brought into [-1, 1)."""
    sv = np.asarray(sc.rp.RxSteeringVec)
    u = -2.0 * np.angle(sv[1] / sv[0]) / np.pi
    return (u + 1.0) % 2.0 - 1.0


def u_distance(a, b):
    """|a - b| on the circle of period 2 of a ULA's dir_u."""
    return np.abs((np.asarray(a) - np.asarray(b) + 1.0) % 2.0 - 1.0)


@functools.lru_cache(maxsize=None)
def oracle_e2e(name):
    """Oracle only: O.mono_static_sensing -> fft2d -> the list's restatement (with snapshots) -> resolve with max_sources = the number of targets.  Shared, read-only."""
    import oracle as O
    import _target_list_restatement as T
    sc = make_e2e(name)
    cf = O.cfar2d_config(sc.rp)
    echo = O.mono_static_sensing(sc.tx_wave, sc.tx_grid.shape, sc.carrier, sc.rp, sc.los, sc.noise, nfft=sc.wave.Nfft)
    _, dbg = O.fft2d(sc.rp, cf, echo, sc.tx_grid, return_debug=True, rdm_fn=O.rdm_explicit)
    rect = (cf.rowRange[0], cf.rowRange[1], cf.colRange[0], cf.colRange[1])
    hr, hc = cf.GuardBandSize[0] + cf.TrainingBandSize[0], cf.GuardBandSize[1] + cf.TrainingBandSize[1]
    fr, fc = rect[0] - hr, rect[2] - hc
    win = dbg.rdm[fr - 1:rect[1] + hr, fc - 1:rect[3] + hc, :].copy()
    t = T.target_list(np.abs(win) ** 2, dbg.detections, fr, fc, rect, sc.rp, lambda r, c: win[r - fr, c - fc, :].T)
    return SimpleNamespace(sc=sc, list=t, truth_u=apparent_u(sc), ref=resolve(t.snapshots, None, len(E2E[name]["velocity"])))


# The restatement's own error against the truth at cycles = 16, in lobes, measured by tests/test_directions_cpu.py::test_two_and_three_sources (which prints it) and kept here
# with the margin of 10 the convergence rate of RELAX asks for; the GPU test adds 1e-6 of a lobe.
MEASURED_LOBES = {"ula16_two": 8.9e-15, "ula64_two": 0.0, "ula256_two": 0.0, "ula16_three": 2.2e-16, "upa2x8_two": 4.4e-16, "upa8x2_two": 1.1e-16,
                  "upa4x4_three": 2.1e-9, "upa16x16_two": 2.2e-16}
