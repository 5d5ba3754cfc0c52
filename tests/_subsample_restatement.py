"""NumPy restatement of include/isac_subsample.h (DESIGN.md section 5 -- project-defined) and the scenes its two test files share.  Nothing here comes from the package
under test.

The estimator (isac_range_refine_dev): direct sums in np.longdouble -- the Doppler contraction over all L symbols, the 17 probes, the peak rule, 40 halvings on the sign of
P' -- plus the fp64 rounding bound the conditioning test holds |P'| against.

The fractional echo (isac_multi_static_sensing_frac_dev), two ways:
  (a) frac_echo_ramp: the definition -- each path's coefficient vector of the INTEGER delay from tests/_multistatic_restatement.py, demodulated by the oracle, times the ramp
      exp(-2 pi j (frac(fc delta / fs) + m_k delta / Nfft)), spread over the receive array;
  (b) frac_echo_physical: no ramp anywhere -- every OFDM symbol of the source, cyclic prefix included, is the sum of its subcarrier exponentials, evaluated at the
      continuous time t - (d + delta) Ts (the previous symbol's sum where that time falls into it), then the Doppler and carrier phases of isac_multistatic.h line 14, then
      the oracle's demodulator.
(a) = (b) while d + delta <= CP / 2 - 1 AND the path has no Doppler shift: with a shift f the demodulated symbol leaks between subcarriers, (a) gives a leaked term the ramp
of the bin it lands on and (b) that of the bin it left; ramp_leak_bound is the size of that."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import oracle as O
from oracle.matlab_compat import kaiser

import _multistatic_restatement as M

_LD = np.longdouble
_CLD = np.clongdouble
_PI_LD = 4 * np.arctan(_LD(1))
N_BISECT = 40
PROBES = 8                                                                  # a side, 1/8 bin apart
U = 2.0 ** -53


def _expj_ld(turns):
    """e^{2 pi j turns} in long double, the turn count reduced modulo 1 first."""
    t = np.asarray(turns, dtype=_LD)
    t = t - np.rint(t)
    return (np.cos(2 * _PI_LD * t) + 1j * np.sin(2 * _PI_LD * t)).astype(_CLD)


# ---------------------------------------------------------------- the estimator
def contract(rx, tx, nu):
    """c[k, a] = sum_l (rx conj(tx))[k, l, a] e^{-2 pi j nu l} in long double."""
    H = np.asarray(rx, dtype=_CLD) * np.conj(np.asarray(tx, dtype=_CLD))
    ph = _expj_ld(-_LD(nu) * np.arange(H.shape[1]).astype(_LD))
    return (H * ph[None, :, None]).sum(axis=1)


def _zd(c, w, n_ifft, rho):
    """(Z_a(rho), D_a(rho)) [A] each: Z = nIFFT^{-1/2} sum_k w_k c e^{2 pi j k rho / nIFFT}, D the same sum with the factor k (Z' = 2 pi j D / nIFFT)."""
    k = np.arange(c.shape[0]).astype(_LD)
    e = _expj_ld(k * _LD(rho) / _LD(n_ifft)) * w.astype(_LD)
    z = c * e[:, None]
    s = np.sqrt(_LD(n_ifft))
    return z.sum(axis=0) / s, (z * k[:, None]).sum(axis=0) / s


def power_ld(c, w, n_ifft, n_fft, rho):
    z, _ = _zd(c, w, n_ifft, rho)
    return (z.real * z.real + z.imag * z.imag).sum() / _LD(n_fft)


def dp_ld(c, w, n_ifft, n_fft, rho):
    """P'(rho) = (2 / nFFT) sum_a Re(conj(Z_a) Z_a') in long double."""
    z, d = _zd(c, w, n_ifft, rho)
    return -(4 * _PI_LD / (_LD(n_fft) * _LD(n_ifft))) * (z.real * d.imag - z.imag * d.real).sum()


def range_refine(rx, tx, n_ifft, n_fft, row, nu, probe_only=False):
    """isac_range_refine_dev restated: status, rho, power [n] and x [A x n] (fp64 values of the long double results), and c: the contracted planes, for the margins."""
    row, nu = np.asarray(row, dtype=np.int64).ravel(), np.asarray(nu, dtype=np.float64).ravel()
    K, _, A = rx.shape
    w = kaiser(K, 3.0)
    n = row.size
    status, rho, pw, x, cs = np.zeros(n, dtype=np.int64), np.zeros(n), np.zeros(n), np.zeros((A, n), dtype=np.complex128), []
    for i in range(n):
        c = contract(rx, tx, nu[i])
        cs.append(c)
        rho0 = float(row[i] - 1)
        r = _LD(rho0)
        if probe_only:
            status[i] = 2
        else:
            rhos = [rho0 + g / PROBES for g in range(-PROBES, PROBES + 1)]
            P = [power_ld(c, w, n_ifft, n_fft, v) for v in rhos]
            maxima = [g for g in range(1, 2 * PROBES) if P[g] > P[g - 1] and P[g] >= P[g + 1]]
            if not maxima:
                status[i] = 1
            else:
                g = max(maxima, key=lambda q: (P[q], -q))                   # the largest P, the lowest g on a tie
                lo, hi = _LD(rhos[g - 1]), _LD(rhos[g + 1])
                for _ in range(N_BISECT):
                    mid = (lo + hi) / 2
                    if dp_ld(c, w, n_ifft, n_fft, mid) > 0:
                        lo = mid
                    else:
                        hi = mid
                r = (lo + hi) / 2
        rho[i] = float(r)
        pw[i] = float(power_ld(c, w, n_ifft, n_fft, r))
        x[:, i] = (_zd(c, w, n_ifft, r)[0] / np.sqrt(_LD(n_fft))).astype(np.complex128)
    return SimpleNamespace(status=status, rho=rho, power=pw, x=x, c=cs)


def probe_margins(c, w, n_ifft, n_fft, row):
    """(has_peak, margin) of step 2 at `row`: margin = the smallest relative amount by which a comparison of the peak rule could flip -- for the chosen maximum its gaps to
    both neighbours and to every other local maximum; without a maximum, for every interior probe the larger of its two deficits."""
    rhos = [float(row - 1) + g / PROBES for g in range(-PROBES, PROBES + 1)]
    P = np.array([float(power_ld(c, w, n_ifft, n_fft, v)) for v in rhos])
    maxima = [g for g in range(1, 2 * PROBES) if P[g] > P[g - 1] and P[g] >= P[g + 1]]
    if maxima:
        g = max(maxima, key=lambda q: (P[q], -q))
        return True, min([(P[g] - P[g - 1]) / P[g], (P[g] - P[g + 1]) / P[g]] + [abs(P[g] - P[q]) / P[g] for q in maxima if q != g])
    return False, min(max(P[g - 1] - P[g], P[g + 1] - P[g]) / P[g] for g in range(1, 2 * PROBES))


def empty_row(rx, tx, n_ifft, n_fft, nu, candidates):
    """The first of `candidates` (rows that hold no tone) on which the 17 probes show no interior maximum, by a margin of 1e-6: a noise-only periodogram has one on most
    rows, and the tests want the row that has none."""
    c, w = contract(rx, tx, nu), kaiser(rx.shape[0], 3.0)
    for row in candidates:
        has_peak, margin = probe_margins(c, w, n_ifft, n_fft, row)
        if not has_peak and margin > 1e-6:
            return int(row)
    raise AssertionError("no candidate row without a maximum")


def dp_rounding_bound(rx, tx, n_ifft, n_fft):
    """A bound on the error of P'(rho), any rho below nIFFT, when the two sums run in fp64 the way the device runs them.  With M_a = sum_k w_k sum_l |H[k, l, a]|, the
    size every term of Z_a is bounded by: the phasor of bin k carries a turn count k rho / nIFFT < K rounded once (2 pi K u of phase), a term of c an L-term sum and
    a phasor of up to L / 2 turns, a lane's sum K / 64 terms and a six-level tree, a product a few roundings: eps = (2 pi K + pi L + K / 64 + L + 32) u relative to M_a
    for Z_a sqrt(nIFFT) and to K M_a for D_a sqrt(nIFFT); |Z_a| sqrt(nIFFT) <= M_a and |D_a| sqrt(nIFFT) <= K M_a.  So |dP'| <= (4 pi / (nFFT nIFFT^2)) 2 eps K sum_a M_a^2."""
    K, Ls, _ = rx.shape
    Ma = (np.abs(rx * np.conj(tx)).sum(axis=1) * kaiser(K, 3.0)[:, None]).sum(axis=0)
    eps = (2 * np.pi * K + np.pi * Ls + K / 64 + Ls + 32) * U
    return float(4 * np.pi / (n_fft * float(n_ifft) ** 2) * 2 * eps * K * (Ma * Ma).sum())


# ---------------------------------------------------------------- the scenes of the estimator: rx = H tx + noise with unit-modulus tx, H a sum of tones
# name -> (K, nIFFT, L, A, n).  Tones: (rho, nu, amplitude); entries: (row, nu) as a list or a target list would give them -- the nearest row, and nu a little off the tone
# (a grid column is up to half a Doppler bin away; the estimator takes nu as given).  An entry with row None: empty_row's pick among rows that hold no tone: status 1.
SHAPES = {"k288_a2": (288, 512, 14, 2, 1), "k300_a3": (300, 512, 14, 3, 5), "k288_l28_a8": (288, 512, 28, 8, 33), "k3276_a4": (3276, 4096, 14, 4, 3)}


def _tone_scene(name):
    K, n_ifft, Ls, A, n = SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "k288_a2":
        tones, entries = [(40.37, 0.11, 1.0)], [(41, 0.11)]
    elif name == "k300_a3":                                                 # two tones on one row at different Dopplers; one row with one tone; the empty row
        tones = [(100.3, 0.21, 1.0), (100.7, -0.17, 0.8), (250.55, 0.05, 0.6)]
        entries = [(101, 0.21), (102, -0.17), (252, 0.05), (251, 0.052), (None, 0.3, range(380, 440))]
    elif name == "k288_l28_a8":                                             # 16 tones, each entered from the row below and the row above it, and the empty-Doppler entry
        tones = [(20.0 + 28.0 * i + 0.1 + 0.05 * i, (-0.4 + 0.05 * i), 1.0 - 0.03 * i) for i in range(16)]
        entries = [(int(np.floor(t[0])) + 1, t[1]) for t in tones] + [(int(np.floor(t[0])) + 2, t[1] + 0.003) for t in tones] + [(None, 0.45, range(3, 18))]
    else:
        tones, entries = [(1500.61, -0.23, 1.0), (2200.37, 0.31, 0.7)], [(1502, -0.23), (2201, 0.31), (None, 0.1, range(2900, 3100))]
    assert len(entries) == n
    k = np.arange(K, dtype=np.float64)[:, None, None]
    l = np.arange(Ls, dtype=np.float64)[None, :, None]
    H = np.zeros((K, Ls, A), dtype=np.complex128)
    for (rho, nu, amp) in tones:
        steer = np.exp(2j * np.pi * rng.random(A))[None, None, :]
        H += amp * np.exp(-2j * np.pi * k * rho / n_ifft) * np.exp(2j * np.pi * nu * l) * steer
    tx = np.exp(2j * np.pi * rng.random((K, Ls, A)))
    noise = 0.05 * (rng.standard_normal((K, Ls, A)) + 1j * rng.standard_normal((K, Ls, A)))
    rx = np.asfortranarray(H * tx + noise)
    tx = np.asfortranarray(tx)
    entries = [e if e[0] is not None else (empty_row(rx, tx, n_ifft, 64, e[1], e[2]), e[1]) for e in entries]
    return SimpleNamespace(name=name, K=K, n_ifft=n_ifft, n_fft=64, L=Ls, A=A, n=n, rx=rx, tx=tx, tones=tones, row=np.array([e[0] for e in entries], dtype=np.int32),
                           nu=np.array([e[1] for e in entries], dtype=np.float64), r_res=1.25)


@functools.lru_cache(maxsize=None)
def tone_scene(name):
    """The scene and the restated estimator on it (``ref``), made once per process and shared; callers must not modify it."""
    s = _tone_scene(name)
    s.ref = range_refine(s.rx, s.tx, s.n_ifft, s.n_fft, s.row, s.nu)
    for arr in (s.rx, s.tx, s.row, s.nu):
        arr.setflags(write=False)
    return s


def single_tone(K, n_ifft, Ls, A, rho, nu, seed=0):
    """A noiseless tone at (rho, nu) with unit-modulus tx: (rx, tx)."""
    rng = np.random.default_rng(seed)
    k = np.arange(K, dtype=np.float64)[:, None, None]
    l = np.arange(Ls, dtype=np.float64)[None, :, None]
    H = np.exp(-2j * np.pi * k * rho / n_ifft) * np.exp(2j * np.pi * nu * l) * np.exp(2j * np.pi * rng.random(A))[None, None, :]
    tx = np.exp(2j * np.pi * rng.random((K, Ls, A)))
    return H * tx, tx


# ---------------------------------------------------------------- the fractional echo
def carrier_turns(fc, fs, delta):
    t = fc * delta / fs                                                    # fp64, as the library forms it
    return t - np.floor(t)


def frac_ramp(n_sc, nfft, fc, fs, delta):
    """exp(-2 pi j (frac(fc delta / fs) + m_k delta / Nfft)) [n_sc], m_k = k - n_sc / 2."""
    m = (np.arange(n_sc) - n_sc // 2).astype(_LD)
    return _expj_ld(-(_LD(carrier_turns(fc, fs, delta)) + m * _LD(delta) / _LD(nfft))).astype(np.complex128)


def frac_echo_ramp(waves, n_sc, nfft, scs, fc, fs, n_ants, paths, frac):
    """(a): sum_p a_p (D_p .* ramp_p), D_p = the oracle's demodulation of path p's coefficient vector at its integer delay.  paths: the tuples of
    _multistatic_restatement.multi_static_channel.  Returns [n_sc x L x n_ants]."""
    out = None
    for (s, d, f, g, b, a), delta in zip(paths, frac):
        coef = M.multi_static_channel(waves, fc, fs, 0.0, 1, [(s, d, f, g, b, np.ones(1))], None)
        D = O.ofdm_demodulate(coef, n_sc, nfft, scs)
        if delta != 0.0:
            D = D * frac_ramp(n_sc, nfft, fc, fs, delta)[:, None, None]
        term = D * np.asarray(a)[None, None, :]
        out = term if out is None else out + term
    return out


def frac_echo_physical(grids, amps, n_sc, nfft, scs, fc, fs, n_ants, paths, frac, T):
    """(b): grids[s] [n_sc x L x A_s], the grid source s's waveform amps[s] * O.ofdm_modulate(grids[s]) was modulated from.  Returns [n_sc x L x n_ants]."""
    n_sym = next(g for g in grids if g is not None).shape[1]
    starts, cps = O.symbol_starts(nfft, scs, n_sym)
    ends = starts + cps + nfft
    m = (np.arange(n_sc) - n_sc // 2).astype(np.float64)
    t_axis = np.arange(T, dtype=np.float64)
    rx = np.zeros((T, n_ants), dtype=np.complex128)
    for (s, d, f, g, b, a), delta in zip(paths, frac):
        gb = np.tensordot(np.asarray(grids[s]), np.asarray(b), axes=([2], [0])) * (amps[s] / nfft)    # [n_sc x L]: the beam's grid, ifft scaling
        tau = t_axis - (d + delta)                                          # continuous source time of every received sample
        x = np.zeros(T, dtype=np.complex128)
        for l in range(n_sym):
            sel = np.flatnonzero((tau >= starts[l]) & (tau < ends[l]))
            if sel.size:
                u = tau[sel] - (starts[l] + cps[l])                         # time into the useful part; negative inside the prefix
                x[sel] = np.exp(2j * np.pi * np.outer(u, m) / nfft) @ gb[:, l]
        # e^{j 2 pi fc (t - d - delta) Ts} e^{-j 2 pi fc t Ts}: the two exponentials at whole samples in fp64, as basicRadarChannel.m:30,73 forms them -- at 1.9e6 turns their
        # arguments are rounded by 1e-9 rad, a rounding the integer-delay restatement under (a) and the device share -- and the fraction's share of the carrier exactly
        ts = 1.0 / fs
        carrier = np.exp(2j * np.pi * fc * ((t_axis - d) * ts)) * np.exp(-2j * np.pi * fc * (t_axis * ts)) * complex(_expj_ld(-_LD(fc) * _LD(delta) / _LD(fs)))
        coef = g * np.exp(2j * np.pi * f * (t_axis * ts)) * carrier * x
        rx += coef[:, None] * np.asarray(a)[None, :]
    return O.ofdm_demodulate(rx, n_sc, nfft, scs)


def ramp_leak_bound(n_sc, nfft, scs, f, delta):
    """The size of the difference of (a) and (b) for a path with Doppler shift f and fraction delta, relative to the path's grid.  The value a subcarrier q bins away
    leaks into a bin has the weight |sin(pi eps) / (Nfft sin(pi (q - eps) / Nfft))| <= eps / (|q| - eps), eps = |f| / SCS, of its own size, and the two ramps differ on
    it by |1 - e^{2 pi j q delta / Nfft}| <= 2 pi |q| delta / Nfft: a term of at most 2 pi eps delta / (Nfft (1 - eps)) whatever q.  A bin collects n_sc - 1 such terms
    from grid values of independent phases (QPSK), so their sum has the rms sqrt(n_sc) times that, relative to the rms of the path's grid; the largest of the 1e4 ... 1e5
    values of a grid lies within 6 rms (a Gaussian sum exceeds 6 sigma once in 5e8), and max|grid| is no smaller than the grid's rms:
        6 sqrt(n_sc) 2 pi eps delta / (Nfft (1 - eps)).
    Independent paths add in power on both sides, so a sum of paths stays within the largest of their bounds."""
    eps = abs(f) / (scs * 1e3)
    return 6 * np.sqrt(n_sc) * 2 * np.pi * eps * delta / (nfft * (1 - eps))


# the frac scenes: Nfft 256, 60 kHz, 11 PRB (cyclic prefix 18 / 26 samples: CP / 2 - 1 = 8), two sources with 2 and 3 elements, 4 receive elements, 3 paths.
# "still": no Doppler shift, d + delta <= 8 -- the scene of the physical reference -- at 700 MHz over 3 symbols.  Why so few turns of the carrier: line 14's two carrier
# exponentials are formed in fp64 at fc t Ts turns each, and for d > 0 their product carries the rounding of both arguments, 2 pi u fc t Ts rad of it, as NOISE from
# sample to sample (for d = 0 the two arguments are the same number and it cancels).  (a) demodulates that noise and then ramps it, (b) lays it on the delayed signal: the two
# differ by the noise itself -- 1e-9 of max|grid| at 3.5 GHz behind 27 symbols (1.8e6 turns), 8e-12 here (3.8e4 turns).  It is the integer delay's rounding, which the
# device shares (tests/test_gpu_multistatic.py holds it to (a)'s integer part), and no property of the fraction.
# "moving": 3.5 GHz, 30 symbols -- symbol 28 has the numerology's second long prefix -- Doppler shifts of both signs, one path with delta = 0 beside the others, a delay
# beyond the prefix -- against (a), the definition, only.
FRAC_NFFT, FRAC_SCS, FRAC_NRB = 256, 60, 11
FRAC_SCENES = {
    "still": dict(fc=0.7e9, L=3, source=(1, 0, 1), shift=(0, 3, 7), frac=(0.37, 0.5, 0.9), doppler=(0.0, 0.0, 0.0)),
    "moving": dict(fc=3.5e9, L=30, source=(0, 1, 1), shift=(2, 40, 5), frac=(0.25, 0.0, 0.999), doppler=(-3100.0, 900.0, 2500.0)),
}


@functools.lru_cache(maxsize=None)
def frac_scene(name):
    kw = FRAC_SCENES[name]
    rng = np.random.default_rng(len(name))
    K, A, a_src = 12 * FRAC_NRB, 4, (2, 3)
    fs = float(FRAC_NFFT * FRAC_SCS * 1e3)
    grids = [np.exp(0.5j * np.pi * rng.integers(0, 4, (K, kw["L"], a))) for a in a_src]
    amps = (1.0, 0.7)
    waves = [np.asfortranarray(amps[s] * O.ofdm_modulate(grids[s], FRAC_NFFT, FRAC_SCS)) for s in range(2)]
    T = waves[0].shape[0]
    P = len(kw["source"])
    tx_st = [np.exp(2j * np.pi * rng.random(a_src[s])) for s in kw["source"]]
    rx_st = np.asfortranarray(np.exp(2j * np.pi * rng.random((A, P))))
    paths = SimpleNamespace(source=np.array(kw["source"], dtype=np.int32), shift=np.array(kw["shift"], dtype=np.int64), doppler=np.array(kw["doppler"]),
                            gain=rng.uniform(0.5, 1.5, P), txSteering=tx_st, rxSteering=rx_st, frac=np.array(kw["frac"]))
    rows = M.path_tuples(paths)
    rp = SimpleNamespace(fc=kw["fc"], fs=fs, N0=2.0, nTxAnts=A)
    ramp = np.asfortranarray(frac_echo_ramp(waves, K, FRAC_NFFT, FRAC_SCS, kw["fc"], fs, A, rows, paths.frac))
    for arr in waves + [ramp]:
        arr.setflags(write=False)
    return SimpleNamespace(K=K, A=A, L=kw["L"], T=T, nfft=FRAC_NFFT, scs=FRAC_SCS, grids=grids, amps=amps, waves=waves, paths=paths, rows=rows, rp=rp, ramp=ramp,
                           carrier=SimpleNamespace(NRBsDL=FRAC_NRB, SubcarrierSpacing=FRAC_SCS), cp=int(O.cp_lengths(FRAC_NFFT, FRAC_SCS, 2)[1]))


@functools.lru_cache(maxsize=None)
def frac_physical(name):
    s = frac_scene(name)
    return frac_echo_physical(s.grids, s.amps, s.K, s.nfft, s.scs, s.rp.fc, s.rp.fs, s.A, s.rows, s.paths.frac, s.T)


# ---------------------------------------------------------------- the end-to-end scene: 24 PRB at 30 kHz (K 288, Nfft = nIFFT 512: one sample is one range bin), 4 elements,
# 28 symbols, two targets whose ranges lie 0.37 and 0.61 of a bin above a bin
E2E_BINS = (7.37, 14.61)                                                    # 72 m and 143 m: inside the detection area, and d + delta inside CP / 2 - 1 = 17
E2E_VELOCITY = (30.0, -40.0)                                              # 1.6 Doppler resolution cells apart over the 28 symbols: each contraction takes the other tone down
E2E_SEED = 4242


@functools.lru_cache(maxsize=None)
def e2e_scene():
    """conftest.make_scene with the two targets placed at E2E_BINS range bins (on the ground, azimuths +12 and -20 degrees)."""
    from conftest import make_scene
    r_res = O.LIGHTSPEED / (2 * 30e3 * 512)
    pos = []
    for bins, azi in zip(E2E_BINS, (12.0, -20.0)):
        R, dz = bins * r_res, 1.5 - 30.0                                    # the gNB stands at (0, 0, 30)
        h = np.sqrt(R * R - dz * dz)
        pos.append((h * np.cos(np.deg2rad(azi)), h * np.sin(np.deg2rad(azi)), 1.5))
    sc = make_scene(n_ants=4, n_slots=2, nrb=24, targets=tuple(pos), velocity=E2E_VELOCITY, seed=31, zero_s_slots=False, with_noise=False, num_slots_param=6)
    assert sc.rp.rRes == r_res and np.allclose(np.asarray(sc.rp.range) / r_res, E2E_BINS, rtol=0, atol=1e-9)
    return sc


def e2e_paths(sc):
    """The two own echoes with floor / frac delays: (rows, frac), the tuples of multi_static_channel at the integer delay and the fractions."""
    own = M.mono_static_paths(sc.rp, sc.los)
    delay = 2.0 * np.asarray(sc.rp.range, dtype=np.float64) / O.LIGHTSPEED * sc.rp.fs
    shift = np.floor(delay).astype(np.int64)
    rows = [(0, int(shift[i]), float(own.doppler[i]), float(own.gain[i]), own.txSteering[i], own.rxSteering[:, i]) for i in range(len(shift))]
    return rows, delay - shift


def e2e_restated_chain():
    """The restated chain: echo (a) + spectral noise of the scene's N0 -> per target, the strongest cell of sum_a |rdm|^2 within two rows of the truth and its Doppler
    column -> the restated estimator at that (row, nu0).  Returns (rho [2], truth [2] in bins, grid rows)."""
    sc = e2e_scene()
    rows, frac = e2e_paths(sc)
    K, nfft = sc.K, sc.wave.Nfft
    echo = frac_echo_ramp([sc.tx_wave], K, nfft, 30, sc.rp.fc, sc.rp.fs, sc.A, rows, frac)
    rng = np.random.default_rng(E2E_SEED)
    echo = echo + np.sqrt(sc.rp.N0 / 2.0) * np.sqrt(nfft) * (rng.standard_normal(echo.shape) + 1j * rng.standard_normal(echo.shape))
    n_ifft, n_fft = int(sc.rp.nIFFT), int(sc.rp.nFFT)
    pmap = (np.abs(O.rdm_explicit(echo, sc.tx_grid, n_ifft, n_fft)) ** 2).sum(axis=2)
    truth = np.asarray(sc.rp.range) / sc.rp.rRes
    row, nu = [], []
    for t in truth:
        r0 = int(round(t)) - 2
        sub = pmap[r0:r0 + 5]
        r, c = np.unravel_index(int(np.argmax(sub)), sub.shape)
        row.append(r0 + r + 1)
        nu.append((c + 1 - n_fft // 2 - 1) / n_fft)
    ref = range_refine(echo, sc.tx_grid, n_ifft, n_fft, row, nu)
    return ref.rho, truth, np.asarray(row)
