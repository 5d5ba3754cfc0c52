"""Extended-precision reference of music2D's range and velocity pseudo-spectra (music2D.m:67-117), fp64 restatements of the reference's formulation and of
the device's (csrc/music.hip: signal_vectors_kernel, music2d_scan_kernel) with their mutants, and the seeded case list shared by
tests/test_music2d_reference_cpu.py and tests/test_gpu_music2d_spectra.py.  TEST INFRASTRUCTURE ONLY.

Inputs.  tx is unit-modulus QPSK; rx[:, :, a] = tx[:, :, a] .* (sum_q alpha_q a_r(r_q) a_v(v_q)^T s_a(theta_q) + sigma g_a W_a) with a_r, a_v the steering
vectors of music2D.m:92-93, s_a the ULA phase of music.m:82 and W_a one noise plane per antenna.  The planes tx_a .* W_a are independent draws made
orthonormal over the K Ls samples, so the noise part of Ra (the covariance of rx itself, music2D.m:57-58) is exactly diag(sigma^2 g_a^2); g_1 = 1, so sigma alone sets the SNR of the H-plane that the two spectra are made
of (H = rx(:,:,1) .* conj(tx(:,:,1)), music2D.m:67-68).  The gains of the OTHER antennas are how a case states its model order: determineNumTargets
(music.m:109-125) returns 1 + the index of the smallest gap between neighbouring ascending eigenvalues of Ra, and with the noise powers NOISE_PATTERN[(A, L)]
times the signal power those eigenvalues lie near (1, 1 + g_2^2, ...) P, the smallest gap where the pattern puts it.  make_case asserts the intended L on
its own Ra, with the smallest gap at most half of the next one.

Reference.  H is formed from the fp64 inputs (what the device reads).  eigen-decomposition of the smaller of H'H and H H' by mpmath's eighe at 40 digits
(order <= 48, exact products for K Ls <= 4096), the L signal vectors of the other side as H v / |H v|, then 1 / |a - sum_i e_i (e_i' a)|^2 -- the projector
of music2D.m:81-82,88-89 on the complement of the signal vectors, which is the noise projector Un Un' -- in np.longdouble (64-bit mantissa; mpmath objects
where long double is fp64, on a shortened scan at K > 512), |.| / max, 20 log10 as music2D.m:111-117.  full_route_mp() is the reference's own route to the
letter, eig of the K x K Rr and of the Ls x Ls Rv and 1 / (a' Un Un' a), all in mpmath: tests/test_music2d_reference_cpu.py holds the two routes together.
An empty noise space (L >= Ls for the velocity, L >= K for the range) is a flat 0 dB spectrum without estimates (include/isac.h).
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np

import _doa_reference as R
from _doa_reference import EXT, _J, _PI, _abs2, _cos, _cplx, _f64, _h, _real, _rint, _sin, to_db  # noqa: F401  (the reference's arithmetic)

C0 = 299792458.0            # physconst('LightSpeed')  music2D.m:35
GRAN = 0.5                  # music2D.m:43-44
FC = 28e9                   # rdrEstParams.fc
TSRI = 5e-5                 # rdrEstParams.Tsri: lambda / (2 Tsri) = 107 m/s unambiguous
SCS_KHZ = 120.0             # bsParams.scs: c / (2 scs) = 1249 m unambiguous
ZONE = ((0.0, 60.0), (-30.0, 30.0))     # cfarEstZone: rMax = 60 -> 122 range steps, vMax = 60 -> 122 velocity steps
TOL_DB = 1e-6

# noise power of antennas 2.. in units of the signal power, by (A, intended L): the eigenvalues of Ra lie near (1, 1 + m_2, ...) P
NOISE_PATTERN = {(4, 1): (3.0, 40.0, 400.0), (4, 2): (30.0, 36.0, 400.0), (4, 3): (40.0, 400.0, 406.0), (3, 1): (3.0, 40.0), (3, 2): (30.0, 36.0)}

# (range m, velocity m/s, azimuth deg, amplitude): on the 0.5 scan grids / off them
ON_GRID = ((12.0, 5.0, 15.0, 1.0), (37.5, -12.5, -40.0, 0.8), (51.0, 21.0, 62.0, 0.6))
OFF_GRID = ((12.23, 5.17, 15.3, 1.0), (37.71, -12.31, -40.6, 0.8), (51.13, 21.29, 62.4, 0.6))
CLOSE = ((20.0, 5.17, 15.3, 1.0), (20.5, -12.31, -40.6, 0.8))       # two targets one range step apart


def rp_music2d(n_ants, zone=ZONE):
    """rp_ula plus what music2D reads."""
    rp = R.rp_ula(n_ants=n_ants)
    rp.fc, rp.Tsri, rp.cfarEstZone = FC, TSRI, np.asarray(zone, dtype=np.float64)
    return rp


def grids(zone=ZONE):
    """(range values [rSteps], velocity values [vSteps]) of music2D.m:41-46,99,105 (exact in fp64)."""
    r_max, v_max = float(zone[0][1]), float(zone[1][1]) * 2.0
    r_steps, v_steps = int(math.floor((r_max + 1) / GRAN)), int(math.floor((v_max + 1) / GRAN))
    return np.arange(r_steps) * GRAN, np.arange(v_steps) * GRAN - v_max / 2.0


def steer64(kind, x, n):
    """music2D.m:92-93 in fp64, left to right: exp(-2j pi scs 2 r n / c), exp(2j pi T 2 v m / lambda).  [n x len(x)]"""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    idx = np.arange(n, dtype=np.float64)[:, None]
    if kind == "r":
        return np.exp(-2j * np.pi * (SCS_KHZ * 1e3) * 2 * x[None, :] * idx / C0)
    return np.exp(2j * np.pi * TSRI * 2 * x[None, :] * idx / (C0 / FC))


@functools.lru_cache(maxsize=None)
def make_case(K, Ls, A, targets, snr_db, L, seed=0, zone=ZONE):
    """One seeded scene: (rx, tx, rp) and what the reference needs.  `targets`: a tuple of (r, v, azimuth, amplitude)."""
    rng = np.random.default_rng(77000 + 1009 * seed + 31 * K + 7 * Ls + A)
    tx = np.exp(0.5j * np.pi * (rng.integers(0, 4, (K, Ls, A)) + 0.5))
    sig = np.zeros((K, Ls, A), dtype=np.complex128)
    for r, v, az, amp in targets:
        plane = amp * steer64("r", r, K)[:, :1] * steer64("v", v, Ls)[:, 0][None, :]
        sig += plane[:, :, None] * R.steering64(A, [az])[:, 0][None, None, :]
    p_sig = float(sum(t[3] ** 2 for t in targets))
    w = rng.standard_normal((K * Ls, A)) + 1j * rng.standard_normal((K * Ls, A))
    w = np.linalg.qr(w)[0] * math.sqrt(K * Ls)                                     # unit sample power, orthogonal planes
    power = np.concatenate([[p_sig / 10.0 ** (snr_db / 10.0)], np.asarray(NOISE_PATTERN[(A, L)]) * p_sig])
    rx = np.asfortranarray(tx * sig + (w * np.sqrt(power)[None, :]).reshape(K, Ls, A, order="F"))     # (W_a = conj(tx_a) .* w_a: |tx| = 1)
    tx = np.asfortranarray(tx)
    g = rx.reshape(K * Ls, A, order="F")
    ra = g.conj().T @ g / (K * Ls)
    wa = np.linalg.eigvalsh(0.5 * (ra + ra.conj().T))
    gaps = np.sort(np.diff(wa))
    from oracle.music import determine_num_targets
    assert determine_num_targets(wa) == L and 2.0 * gaps[0] <= gaps[1], ("model order", (K, Ls, A), L, wa)
    r_grid, v_grid = grids(zone)
    return SimpleNamespace(K=K, Ls=Ls, A=A, L=L, snr_db=snr_db, targets=targets, rx=rx, tx=tx, rp=rp_music2d(A, zone), zone=zone, Ra=ra, r_grid=r_grid,
                           v_grid=v_grid, name=f"K{K}_Ls{Ls}_A{A}_Q{len(targets)}_L{L}_{snr_db:g}dB_s{seed}")


# ---------------------------------------------------------------------------------------------------------------- the case list
def _c(K, Ls, A, targets, snr_db, L, seed=0):
    return (K, Ls, A, tuple(targets), float(snr_db), L, seed)


def _high_snr(K, Ls, A):
    return [_c(K, Ls, A, tg[:2], snr, 2, seed) for snr in (60, 100) for seed, tg in ((1, ON_GRID), (2, OFF_GRID))]


CASES = {
    "base": [_c(24, 14, 4, OFF_GRID[:2], 10, 2), _c(24, 14, 4, OFF_GRID[:2], 30, 3)] + _high_snr(24, 14, 4),
    "K_lt_Ls": [_c(12, 28, 4, OFF_GRID[:1], 10, 1), _c(12, 28, 4, OFF_GRID[:1], 30, 2)],
    "wave": [_c(63, 14, 4, OFF_GRID[:2], 10, 2), _c(63, 14, 4, ON_GRID[:2], 30, 2), _c(64, 14, 4, OFF_GRID, 10, 3), _c(64, 14, 4, OFF_GRID, 30, 3),
             _c(65, 15, 4, OFF_GRID[:1], 10, 1), _c(65, 15, 4, ON_GRID[:1], 30, 1)],
    "block": [_c(255, 14, 4, OFF_GRID, 10, 3), _c(255, 14, 4, ON_GRID, 30, 3), _c(256, 14, 4, OFF_GRID[:2], 10, 2), _c(256, 14, 4, OFF_GRID[:2], 30, 2),
              _c(257, 15, 4, OFF_GRID[:2], 10, 3), _c(257, 15, 4, OFF_GRID[:2], 30, 2)] + _high_snr(256, 14, 4),
    "Ls65": [_c(48, 65, 4, OFF_GRID[:2], 10, 2), _c(48, 65, 4, OFF_GRID[:2], 30, 2)] + _high_snr(48, 65, 4),
    "A3": [_c(300, 14, 3, CLOSE, 10, 2), _c(300, 14, 3, CLOSE, 30, 2)],
    "named_K": [_c(3276, 28, 4, OFF_GRID, 10, 3), _c(3276, 28, 4, OFF_GRID, 30, 3)],
}
EMPTY_NOISE_SPACE = _c(24, 2, 4, OFF_GRID[:2], 30, 2)      # L = 2 >= Ls = 2: no velocity noise vector
ALL_CASES = [(group, args) for group, lst in CASES.items() for args in lst]


def case_id(args):
    K, Ls, A, targets, snr, L, seed = args
    return f"{K}x{Ls}x{A}-Q{len(targets)}-L{L}-{snr:g}dB-s{seed}"


# ---------------------------------------------------------------------------------------------------------------- the reference
def _to_mp(x):
    """A long double (or fp64) scalar as an mpmath number, exactly."""
    import mpmath
    hi = float(x)
    return mpmath.mpf(hi) + mpmath.mpf(float(x - hi))


def _conj(x):
    return np.conj(x) if EXT else _h(x).T


def _mp_gram(h, cols):
    """H'H (cols) or H H' of the extended-precision H as an mpmath matrix: exact products and sums for K Ls <= 4096, long double sums beyond."""
    import mpmath
    m = h if cols else _h(h)
    n = m.shape[1]
    to = (lambda z: mpmath.mpc(_to_mp(z.real), _to_mp(z.imag))) if EXT else (lambda z: z)
    if m.size <= 4096 or not EXT:
        colv = [[to(z) for z in m[:, j]] for j in range(n)]
        return mpmath.matrix([[mpmath.fsum(x.conjugate() * y for x, y in zip(colv[i], colv[j])) for j in range(n)] for i in range(n)])
    g = _h(m) @ m
    return mpmath.matrix([[to(g[i, j]) for j in range(n)] for i in range(n)])


def _steer_ext(kind, x, n):
    """The steering vectors of music2D.m:92-93 in the reference's arithmetic: the phase is reduced in turns before it meets pi.  [n x len(x)]"""
    import mpmath
    with mpmath.workdps(40):
        if kind == "r":
            per = -(mpmath.mpf(SCS_KHZ) * 1000 * 2) / mpmath.mpf(C0)                          # turns per metre and index
        else:
            per = (mpmath.mpf(TSRI) * 2) * mpmath.mpf(FC) / mpmath.mpf(C0)                    # turns per m/s and index  (lambda = c / fc)
        per = R._from_mp(mpmath.matrix([[per]]), cplx=False)[0, 0]
    t = (_real(np.asarray(x, dtype=np.float64))[None, :] * per) * _real(np.arange(n, dtype=np.float64))[:, None]
    t = (t - _rint(t)) * (2 * _PI)
    return _cplx(_cos(t)) + _cplx(_sin(t)) * _J


def _residual_spectrum(e, a):
    """1 / |a - sum_i e_i (e_i' a)|^2 per column of a, for (near-)orthonormal columns e; the projection is applied twice (the second pass removes what the
    rounding of the first left in the span of e)."""
    r = a
    for _ in range(2):
        r = r - e @ (_h(e) @ r)
    return 1 / _abs2(r).sum(axis=0)


@functools.lru_cache(maxsize=None)
def reference(args):
    """SimpleNamespace(case, PrdB, PvdB, r_idx, v_idx): the reference spectra of one case at the scan points r_idx / v_idx (all of them wherever long double
    is the x87 format)."""
    import mpmath
    c = make_case(*args)
    K, Ls, L = c.K, c.Ls, c.L
    h = _cplx(c.rx[:, :, 0]) * _conj(_cplx(c.tx[:, :, 0]))                # music2D.m:67-68 on the fp64 inputs, in the reference's arithmetic
    cols = Ls <= K                                          # eigenproblem on H'H [Ls x Ls], else on H H' [K x K]
    n_vec = min(L, K, Ls)
    with mpmath.workdps(40):
        e, q = mpmath.eighe(_mp_gram(h, cols))
        w, z = R._from_mp(e, cplx=False)[:, 0], R._from_mp(q)
    order = np.argsort(-_f64(w), kind="stable")[:n_vec]
    z = z[:, order]
    other = (h @ z) if cols else (_h(h) @ z)                # the signal vectors of the other side, H v (or H' u), normalised
    other = other / (_abs2(other).sum(axis=0) ** 0.5)[None, :]
    u, v = (other, z) if cols else (z, other)               # u: of Rr [K], v: of H'H [Ls]; Rv = conj(H'H) / K has the vectors conj(v)
    r_idx, v_idx = np.arange(c.r_grid.size), np.arange(c.v_grid.size)
    if not EXT and K > 512:                                 # mpmath objects: a shortened scan
        r_idx, v_idx = r_idx[::8], v_idx[::8]
    if L >= K:
        pr_db = np.zeros(r_idx.size)
    else:
        pr_db = to_db(_residual_spectrum(u, _steer_ext("r", c.r_grid[r_idx], K)))
    if L >= Ls:
        pv_db = np.zeros(v_idx.size)
    else:
        pv_db = to_db(_residual_spectrum(_conj(v), _steer_ext("v", c.v_grid[v_idx], Ls)))
    return SimpleNamespace(case=c, PrdB=pr_db, PvdB=pv_db, r_idx=r_idx, v_idx=v_idx)


def full_route_mp(args):
    """music2D.m:71-117 to the letter in mpmath at 40 digits: eig of the K x K Rr and of the Ls x Ls Rv, the noise vectors beyond the L largest,
    1 / (a' Un Un' a), |.| / max, 20 log10.  For small K."""
    import mpmath
    c = make_case(*args)
    K, Ls, L = c.K, c.Ls, c.L
    out = []
    with mpmath.workdps(40):
        h = mpmath.matrix([[mpmath.mpc(c.rx[k, l, 0]) * mpmath.mpc(c.tx[k, l, 0]).conjugate() for l in range(Ls)] for k in range(K)])     # :67-68
        rr = h * h.H / Ls                                                                                                             # :71
        rv = h.T * h.conjugate() / K                                                                                                  # :72
        two_pi_j = 2 * mpmath.pi * mpmath.mpc(0, 1)
        scs, t_sym, lam = mpmath.mpf(SCS_KHZ) * 1000, mpmath.mpf(TSRI), mpmath.mpf(C0) / mpmath.mpf(FC)
        for mat, n, grid, steer in ((rr, K, c.r_grid, lambda x, i: mpmath.exp(-two_pi_j * scs * 2 * x * i / mpmath.mpf(C0))),            # :92
                                    (rv, Ls, c.v_grid, lambda x, i: mpmath.exp(two_pi_j * t_sym * 2 * x * i / lam))):                    # :93
            e, q = mpmath.eighe(mat)
            order = sorted(range(n), key=lambda i: -e[i])                                                                               # :79-80
            noise = [q[:, i] for i in order[L:]]                                                                                        # :81
            p = []
            for x in grid:
                a = mpmath.matrix([steer(mpmath.mpf(float(x)), i) for i in range(n)])
                den = mpmath.fsum(abs((un.H * a)[0]) ** 2 for un in noise)                                                              # :101
                p.append(1 / den if den != 0 else mpmath.inf)
            if not noise:
                out.append(np.zeros(len(grid)))
                continue
            mx = max(p)
            out.append(np.array([float(20 * mpmath.log10(v / mx)) for v in p]))                                                         # :111-117
    return out[0], out[1]


# ---------------------------------------------------------------------------------------------------------------- fp64 restatements + mutants
FORMS = ("reference", "gram_difference", "gram_residual")
MUTANTS = ("range_phase_sign", "velocity_phase_sign", "velocity_no_conj", "L_plus_1", "L_minus_1", "no_vmax_offset", "shift_one_step", "norm_Ls_for_K",
           "fp32_phase", "scs_1e-7", "drop_partial_sum", "norm_mean")


def _block_sum(terms, mutant):
    """sum over axis 0 the way a 256-thread block sums it: thread t takes n = t, t + 256, ...; 64 lanes per wave, four wave partials.
    `drop_partial_sum` loses the second wave's."""
    n = terms.shape[0]
    wave = (np.arange(n) % 256) // 64
    parts = [terms[wave == k].sum(axis=0) for k in range(4)]
    if mutant == "drop_partial_sum":
        parts[1] = parts[1] * 0
    return parts[0] + parts[1] + parts[2] + parts[3]


def restatement(args, form="reference", mutant=None):
    """(PrdB, PvdB) in plain fp64 NumPy.  form "reference": music2D.m:71-117, eig of Rr and Rv and 1 / (a' Un Un' a) (oracle.music.music2d's arithmetic);
    "gram_difference": eig of G / K = H'H / K, u = H v / sqrt(K mu), 1 / (N - sum_i |e_i' a|^2) -- the device's scan before the comparison on the
    device was made; "gram_residual": the same vectors, 1 / sum_n |a_n - sum_i e_i[n] (e_i' a)|^2 -- what music2d_scan_kernel computes.
    `mutant`: one of MUTANTS, a wrong kernel that the comparison must reject."""
    c = make_case(*args)
    K, Ls, L = c.K, c.Ls, c.L
    L = L + 1 if mutant == "L_plus_1" else L - 1 if mutant == "L_minus_1" else L
    h = c.rx[:, :, 0] * np.conj(c.tx[:, :, 0])
    scs = SCS_KHZ * 1e3 * ((1 + 1e-7) if mutant == "scs_1e-7" else 1.0)
    lam = C0 / FC
    v_max = float(c.zone[1][1]) * 2.0
    shift = GRAN if mutant == "shift_one_step" else 0.0
    r_vals = c.r_grid + shift
    v_vals = np.arange(c.v_grid.size) * GRAN + shift - (0.0 if mutant == "no_vmax_offset" else v_max / 2.0)
    arg_r = (((((-2.0 * np.pi) * scs) * 2.0) * r_vals)[None, :] * np.arange(K, dtype=np.float64)[:, None]) / C0          # the device's order; fp64 product
    arg_v = (((((2.0 * np.pi) * TSRI) * 2.0) * v_vals)[None, :] * np.arange(Ls, dtype=np.float64)[:, None]) / lam        # order cannot matter at 1e-8 dB
    if mutant == "fp32_phase":
        arg_r, arg_v = arg_r.astype(np.float32).astype(np.float64), arg_v.astype(np.float32).astype(np.float64)
    if mutant == "range_phase_sign":
        arg_r = -arg_r
    if mutant == "velocity_phase_sign":
        arg_v = -arg_v
    a_r, a_v = np.cos(arg_r) + 1j * np.sin(arg_r), np.cos(arg_v) + 1j * np.sin(arg_v)
    if form == "reference":
        rr, rv = h @ h.conj().T / Ls, h.T @ h.conj() / K
        spectra = []
        for mat, a in ((0.5 * (rr + rr.conj().T), a_r), (0.5 * (rv + rv.conj().T), a_v)):
            w, q = np.linalg.eigh(mat)
            un = q[:, np.argsort(-w, kind="stable")[L:]]
            spectra.append(1.0 / (np.abs(un.conj().T @ a) ** 2).sum(axis=0) if un.shape[1] else np.ones(a.shape[1]))
    else:
        g = h.conj().T @ h / K
        mu, vv = np.linalg.eigh(0.5 * (g + g.conj().T))
        top = np.argsort(-mu, kind="stable")[:min(L, Ls)]
        u = (h @ vv[:, top]) / np.sqrt((Ls if mutant == "norm_Ls_for_K" else K) * mu[top])[None, :]
        e_v = vv[:, top] if mutant == "velocity_no_conj" else vv[:, top].conj()
        spectra = []
        for e, a, n, empty in ((u, a_r, K, L >= K), (e_v, a_v, Ls, L >= Ls)):
            if empty:
                spectra.append(np.ones(a.shape[1]))
                continue
            y = np.stack([_block_sum(e[:, i].conj()[:, None] * a, mutant) for i in range(e.shape[1])]) if e.shape[1] else np.zeros((0, a.shape[1]))
            if form == "gram_difference":
                spectra.append(1.0 / (n - (np.abs(y) ** 2).sum(axis=0)))
            else:
                spectra.append(1.0 / _block_sum(np.abs(a - e @ y) ** 2, None))
    out = []
    for p in spectra:
        p = np.abs(p)
        with np.errstate(divide="ignore"):
            out.append(20.0 * np.log10(p / (p.mean() if mutant == "norm_mean" else p.max())))
    return out[0], out[1]


deviation, accept = R.deviation, R.accept
