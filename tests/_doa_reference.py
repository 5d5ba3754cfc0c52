"""Extended-precision reference of the ULA direction-finding spectra (music.m:82-96, digitalBF.m:55-86, mvdrBF.m:55-86), the fp64 NumPy
restatement of what music_scan_kernel computes (csrc/music.hip), its mutants, and the case list shared by tests/test_doa_spectra_cpu.py and
tests/test_gpu_doa_spectra.py.  TEST INFRASTRUCTURE ONLY.

The reference owes nothing to the code under test:

* arithmetic: np.longdouble where it is the 64-bit-mantissa x87 format (eps 1.08e-19 < 1e-18), mpmath at 40 digits (object arrays) elsewhere;
* sind exact at multiples of 90 (the fold of oracle.matlab_compat, which is exact in fp64, then sin / cos of a first-octant angle in extended
  precision); the steering phase 2 pi n d sind(phi) is reduced in TURNS before it meets pi, so its error is that of pi, not of the argument;
* PRESCRIBED eigenstructure, any A: eigenvalues w and a matrix V that is unitary in extended precision (fp64 QR, then two Newton-Schulz
  re-orthonormalisations V <- V (3 I - V'V) / 2 in extended precision; max |V'V - I| <= 1e-18 asserted).  Ra = V diag(w) V' is formed in
  extended precision and rounded to fp64 -- that matrix is what the device and the oracle receive -- and the spectra come from (w, V) directly:
  MUSIC from the A - L smallest, DBF from sum w_i |v_i'a|^2, MVDR from 1 / (sum |v_i'a|^2 / w_i + eps).  No inverse, no eigendecomposition;
* PHYSICAL sample covariances, A <= 16: mpmath's own eighe (MUSIC) and inverse (MVDR) at 40 digits, DBF from Ra itself;
* any Hermitian Ra with a known split (the chain at A = 65): the signal projector as (I + sign(Ra - mu I)) / 2, the matrix sign by Newton-Schulz
  products in extended precision, mu anywhere inside the gap (trace = L asserted).

What rounding Ra to fp64 (and handing an fp64 eigensolver that matrix) may cost is a condition on the INPUTS, kept by every case below and
asserted in tests/test_doa_spectra_cpu.py: cond(Ra) <= 1e7 for MVDR; for MUSIC a gap (w[L-1] - w[L]) >= 1e-3 w[0] at the split and
min over the scan of a'Uan Uan'a >= 1e-6 A.  Under them the fp64 formulations stay within 1e-8 dB of this reference at every scan point.
"""
from __future__ import annotations

import functools
import math
from types import SimpleNamespace

import numpy as np

EPS = 2.0 ** -52            # eps(1): music.m:90, mvdrBF.m:72
D = 0.5                     # music.m:12
EXT = bool(np.finfo(np.longdouble).eps < 1e-18)

if EXT:
    _R, _C = np.longdouble, np.clongdouble
    _PI = _R("3.14159265358979323846264338327950288")
    _cos, _sin, _rint = np.cos, np.sin, np.rint

    def _real(x):
        return np.asarray(x, dtype=_R)

    def _cplx(x):
        return np.asarray(x, dtype=_C)

    def _f64(x):
        return np.asarray(x, dtype=np.float64)

    def _abs2(z):
        return z.real * z.real + z.imag * z.imag

    def _absr(x):
        return np.abs(x)

    _J = 1j
else:  # pragma: no cover  (platforms whose long double is the fp64 format): object arrays of mpmath numbers
    import mpmath
    mpmath.mp.dps = 40
    _PI = +mpmath.mp.pi
    _J = mpmath.mpc(0, 1)

    def _each(fn, x):
        return np.asarray(np.frompyfunc(fn, 1, 1)(np.asarray(x, dtype=object)), dtype=object)

    def _cos(x):
        return _each(mpmath.cos, x)

    def _sin(x):
        return _each(mpmath.sin, x)

    def _rint(x):
        return _each(lambda v: mpmath.floor(v + mpmath.mpf(1) / 2), x)

    def _real(x):
        return _each(lambda v: v if isinstance(v, mpmath.mpf) else mpmath.mpf(float(v)), x)

    def _cplx(x):
        return _each(lambda v: mpmath.mpc(v) if isinstance(v, (mpmath.mpf, mpmath.mpc)) else mpmath.mpc(complex(v)), x)

    def _f64(x):
        return np.asarray(_each(float, x), dtype=np.float64)

    def _abs2(z):
        return _each(lambda v: mpmath.re(v) ** 2 + mpmath.im(v) ** 2, z)

    def _absr(x):
        return _each(abs, x)


def _h(m):
    """Conjugate transpose in the reference's arithmetic."""
    return np.conj(m).T if EXT else _each(lambda v: v.conjugate(), m).T


def scan_angles(gran=1.0, scale=360.0):
    """music.m:79,88: floor((aMax + 1) / aGran) angles (a - 1) aGran - aMax / 2 (exact in fp64 for the grids used here)."""
    steps = int(math.floor((scale + 1.0) / gran))
    return np.arange(steps, dtype=np.float64) * gran - scale / 2.0


def rp_ula(gran=1.0, scale=360.0, n_ants=16):
    """The fields of radarEstParams that the ULA DoA calls read."""
    return SimpleNamespace(nIFFT=4096, nFFT=64, rRes=1.0, vRes=1.0, antennaType=SimpleNamespace(kind="ula", numElements=n_ants),
                           azimuthScanScale=scale, azimuthScanGranularity=gran, elevationScanScale=180, elevationScanGranularity=1)


def sind_ext(x):
    """sind in the reference's arithmetic; exact at multiples of 90."""
    x = np.fmod(np.asarray(x, dtype=np.float64), 360.0)
    x = np.where(x > 180.0, x - 360.0, x)
    x = np.where(x < -180.0, x + 360.0, x)
    x = np.where(x > 90.0, 180.0 - x, x)
    x = np.where(x < -90.0, -180.0 - x, x)                                # (all exact in fp64)
    ax = np.abs(x)
    k = _PI / 180
    small, big = _sin(_real(np.where(ax <= 45.0, x, 0.0)) * k), _cos(_real(np.where(ax <= 45.0, 0.0, 90.0 - ax)) * k) * _real(np.sign(x))
    return np.where(ax <= 45.0, small, big)


def steering(n_ants, angles):
    """a(phi)[n] = exp(-2j pi n d sind(phi)) (music.m:82), [n_ants x steps]."""
    t = _real(np.arange(n_ants, dtype=np.float64) * D)[:, None] * sind_ext(angles)[None, :]     # turns
    t = (t - _rint(t)) * (2 * _PI)
    return _cplx(_cos(t)) - _cplx(_sin(t)) * _J


def to_db(p):
    """music.m:94-96: 20 log10(|p| / max |p|), as fp64 (the ratio is rounded once, the logarithm is fp64's)."""
    p = _absr(p)
    with np.errstate(divide="ignore"):
        return 20.0 * np.log10(_f64(p / p.max()))


def projections(v, angles):
    """|v_i' a(phi)|^2 [A x steps] for the columns of v."""
    return _abs2(_h(v) @ steering(v.shape[0], angles))


def spectra_from_projections(w, y, method, n_sig=None):
    """The dB spectrum of one method from eigenvalues w (DESCENDING, extended) and y = projections(V, angles).  method 0: MUSIC with n_sig signal
    vectors (n_sig >= A: empty noise space, flat 0 dB -- music.m:28); 1: digitalBF; 2: mvdrBF."""
    if method == 0:
        q = y[n_sig:].sum(axis=0) if n_sig < y.shape[0] else y[:1].sum(axis=0) * 0
        return to_db(1 / (q + _real(EPS)))
    if method == 1:
        return to_db((w[:, None] * y).sum(axis=0))
    return to_db(1 / ((y / w[:, None]).sum(axis=0) + _real(EPS)))


# ---------------------------------------------------------------------------------------------------------------- prescribed eigenstructure
SOURCES = (15.3, -40.6)     # off the 1 degree grid: the MUSIC quadratic form keeps a floor at every scan point


def steering64(n_ants, angles_deg):
    return np.exp(-2j * np.pi * np.arange(n_ants)[:, None] * D * np.sin(np.deg2rad(np.asarray(angles_deg, dtype=np.float64)))[None, :])


@functools.lru_cache(maxsize=None)
def prescribed_basis(n_ants, seed=0):
    """V [A x A], unitary in extended precision; its first min(2, A - 1) columns span the steering vectors of SOURCES (to fp64 rounding)."""
    rng = np.random.default_rng(1000 + 7 * n_ants + seed)
    n_src = min(len(SOURCES), n_ants - 1)
    m = rng.standard_normal((n_ants, n_ants)) + 1j * rng.standard_normal((n_ants, n_ants))
    m[:, :n_src] = steering64(n_ants, SOURCES[:n_src])
    q, _ = np.linalg.qr(m)
    v = _cplx(q)
    eye = _cplx(np.eye(n_ants))
    for _ in range(2):
        v = v @ (eye * 3 - _h(v) @ v) / 2
    err = _f64(_absr(_abs2(_h(v) @ v - eye))).max() ** 0.5
    assert err <= 1e-18, (n_ants, err)
    return v, n_src


def prescribed_eigenvalues(n_ants, n_src, spread):
    """Descending: the signal values 1, 0.75, then the noise values evenly spaced from 0.5 down to 1 / spread (every split has a gap >= 0.4 / (A - 3))."""
    k = n_ants - n_src
    noise = np.linspace(0.5, 1.0 / spread, k) if k > 1 else np.array([1.0 / spread])
    return np.concatenate([[1.0, 0.75][:n_src], noise]) if n_ants > 1 else np.ones(1)


@functools.lru_cache(maxsize=None)
def prescribed_case(n_ants, spread, seed=0):
    """Ra (fp64, Hermitian, column-major) = V diag(w) V' formed in extended precision, with w, V and the source count."""
    v, n_src = prescribed_basis(n_ants, seed)
    w = _real(prescribed_eigenvalues(n_ants, n_src, spread))
    r = (v * w[None, :]) @ _h(v)
    r = (r + _h(r)) / 2
    ra = np.asfortranarray(np.asarray(r if EXT else _each(complex, r), dtype=np.complex128))
    assert np.array_equal(ra, ra.conj().T)
    return SimpleNamespace(ra=ra, w=w, v=v, n_src=n_src, A=n_ants, spread=spread)


@functools.lru_cache(maxsize=None)
def prescribed_projections(n_ants, seed=0, gran=1.0, scale=360.0):
    return projections(prescribed_basis(n_ants, seed)[0], scan_angles(gran, scale))


def prescribed_spectrum(case, method, n_sig=None, gran=1.0, scale=360.0, seed=0):
    return spectra_from_projections(case.w, prescribed_projections(case.A, seed, gran, scale), method, n_sig)


def lmax_subspace(a):
    """Signal vectors music_subspace_kernel holds (csrc/music.hip, isac_music_subspace_dev); one more takes the automatic fall-back."""
    return max(1, min(32 if a <= 128 else 16, 122880 // (32 * a)))


ARRAY_SIZES = (1, 2, 3, 5, 16, 64, 65, 129, 256, 320)     # below isac_eigh_top's range | small | default | one-workgroup / distributed
SPREADS = (1e1, 1e4, 1e7)                                 # tridiagonalisation boundary | top of the subspace route | full eigendecomposition only
MUSIC_SPREAD = 1e4                                        # the whole numDets list runs on this one; the true source count on every spread


def music_num_dets(a, n_src):
    """1, the true source count, one past the subspace kernel's capacity, A - 1, and the empty noise space (A, A + 4)."""
    return sorted({1, max(n_src, 1), min(lmax_subspace(a) + 1, max(a - 1, 1)), max(a - 1, 1), a, a + 4})


# ---------------------------------------------------------------------------------------------------------------- physical covariances (mpmath)
def sample_cov(seed, a, angles_deg, snr, n):
    """Sample covariance of off-grid sources plus unit noise, built like _sample_cov of tests/test_gpu_music_subspace.py."""
    rng = np.random.default_rng(seed)
    sg = steering64(a, angles_deg)
    q = sg.shape[1]
    s = (rng.standard_normal((q, n)) + 1j * rng.standard_normal((q, n))) * np.sqrt(np.asarray(snr, dtype=np.float64))[:, None]
    x = sg @ s + (rng.standard_normal((a, n)) + 1j * rng.standard_normal((a, n)))
    ra = x @ x.conj().T / n
    return np.asfortranarray(0.5 * (ra + ra.conj().T))


# name -> (seed, A, source angles, per-source SNR, snapshots).  "close3": two sources 3 degrees apart -- the three methods' peak lists differ.
PHYSICAL = {
    "a4": (41, 4, (23.4, -51.7), (100.0, 30.0), 64),
    "a8": (42, 8, (23.4, -51.7), (1e3, 1e2), 200),
    "a16": (43, 16, (15.3, -40.6), (1e4, 1e3), 500),
    "close3": (47, 16, (10.4, 13.4), (10.0, 10.0), 400),
}


def _from_mp(m, cplx=True):
    import mpmath
    conv = (lambda v: _C(_R(mpmath.nstr(mpmath.re(v), 30)) + 1j * _R(mpmath.nstr(mpmath.im(v), 30)))) if cplx else (lambda v: _R(mpmath.nstr(v, 30)))
    if not EXT:  # pragma: no cover
        conv = (lambda v: mpmath.mpc(v)) if cplx else (lambda v: mpmath.mpf(v))
    out = np.empty((m.rows, m.cols), dtype=_C if (EXT and cplx) else (_R if EXT else object))
    for i in range(m.rows):
        for j in range(m.cols):
            out[i, j] = conv(m[i, j])
    return out


def mp_eigh_desc(ra):
    """(w descending, V) of the fp64 matrix ra by mpmath's eighe at 40 digits, in the reference's arithmetic."""
    import mpmath
    with mpmath.workdps(40):
        e, q = mpmath.eighe(mpmath.matrix(np.asarray(ra).tolist()))
        w, v = _from_mp(e, cplx=False)[:, 0], _from_mp(q)
    order = np.argsort(-_f64(w), kind="stable")
    return w[order], v[:, order]


def mp_inverse(ra):
    import mpmath
    with mpmath.workdps(40):
        return _from_mp(mpmath.inverse(mpmath.matrix(np.asarray(ra).tolist())))


def quadratic_forms(mat, n_ants, angles):
    """real(a' M a) per scan point."""
    s = steering(n_ants, angles)
    z = (_h(s).T * (mat @ s)).sum(axis=0)
    return z.real if EXT else _each(mpmath.re, z)


@functools.lru_cache(maxsize=None)
def physical_case(name):
    seed, a, ang, snr, n = PHYSICAL[name]
    ra = sample_cov(seed, a, ang, snr, n)
    w, v = mp_eigh_desc(ra)
    return SimpleNamespace(name=name, ra=ra, A=a, n_src=len(ang), w=w, v=v, inv=mp_inverse(ra))


def physical_spectrum(case, method, n_sig=None, gran=1.0, scale=360.0):
    """MUSIC from mpmath's eigenvectors, DBF from Ra itself, MVDR from mpmath's inverse."""
    angles = scan_angles(gran, scale)
    if method == 0:
        return spectra_from_projections(case.w, projections(case.v, angles), 0, n_sig)
    if method == 1:
        return to_db(quadratic_forms(_cplx(case.ra), case.A, angles))
    return to_db(1 / (quadratic_forms(case.inv, case.A, angles) + _real(EPS)))


# ---------------------------------------------------------------------------------------------------------------- any Ra with a known split
def sign_projector_music(ra, n_sig, gran=1.0, scale=360.0):
    """MUSIC dB spectrum of the fp64 Hermitian ra with n_sig signal vectors, 0 < n_sig < A, without an eigendecomposition: the signal projector is
    (I + sign(Ra - mu I)) / 2 with mu inside the gap between the n_sig-th and the next eigenvalue (fp64 eigvalsh only LOCATES the gap: every mu inside
    it gives the same projector), the sign function by the Newton-Schulz iteration X <- X (3 I - X^2) / 2 in the reference's arithmetic."""
    ra = np.asarray(ra, dtype=np.complex128)
    n = ra.shape[0]
    wd = np.linalg.eigvalsh(ra)[::-1]
    mu = 0.5 * (wd[n_sig - 1] + wd[n_sig])
    eye = _cplx(np.eye(n))
    x = _cplx(ra) - eye * _real(mu)
    x = x / _real(1.01 * max(wd[0] - mu, mu - wd[-1]))                      # spectrum inside (-1, 1), nothing closer to 0 than the half gap
    for it in range(200):
        x2 = x @ x
        if _f64(_absr(_abs2(x2 - eye))).max() ** 0.5 < 1e-17:
            break
        x = x @ (eye * 3 - x2) / 2
        x = (x + _h(x)) / 2
    else:
        raise AssertionError("matrix sign iteration did not converge")
    p_noise = (eye - x) / 2
    tr = float(np.trace(_f64(_each(mpmath.re, p_noise)) if not EXT else _f64(p_noise.real)))
    assert abs(tr - (n - n_sig)) < 1e-9, (tr, n, n_sig)
    return to_db(1 / (quadratic_forms(p_noise, n, scan_angles(gran, scale)) + _real(EPS)))


# ---------------------------------------------------------------------------------------------------------------- fp64 restatement of the kernel + mutants
MUTANTS = ("swap_dbf_mvdr", "mvdr_weighted_by_w", "L_plus_1", "L_minus_1", "fp32_phase", "d_1e-7", "phase_sign", "norm_mean", "shift_one_step")


def restatement(method, ra, n_sig=None, gran=1.0, scale=360.0, mutant=None):
    """What music_scan_kernel's full-eigendecomposition body and the host's dB step compute, in plain fp64 NumPy: eigenpairs of Ra, steering phases
    ((-2 pi m) d) sind(phi) left to right, weighted sums of |v_i'a|^2 over the eigenpairs (weights: noise indicator / w / 1 / w), |.|, / max, 20 log10.
    `mutant`: one of MUTANTS -- a wrong kernel the comparison must reject (tests/test_doa_spectra_cpu.py)."""
    from oracle.matlab_compat import sind
    ra = np.asarray(ra, dtype=np.complex128)
    a = ra.shape[0]
    if mutant == "swap_dbf_mvdr" and method in (1, 2):
        method = 3 - method
    if mutant == "L_plus_1":
        n_sig += 1
    if mutant == "L_minus_1":
        n_sig -= 1
    w, v = np.linalg.eigh(ra)
    angles = scan_angles(gran, scale)
    if mutant == "shift_one_step":
        angles = angles + gran
    d = D * (1 + 1e-7) if mutant == "d_1e-7" else D
    arg = (((-2.0 * np.pi) * np.arange(a, dtype=np.float64)) * d)[:, None] * sind(angles)[None, :]
    if mutant == "fp32_phase":
        arg = arg.astype(np.float32).astype(np.float64)
    if mutant == "phase_sign":
        arg = -arg
    y = np.abs(v.conj().T @ (np.cos(arg) + 1j * np.sin(arg))) ** 2
    if method == 0:
        rank = np.empty(a, dtype=np.int64)
        rank[np.argsort(-w, kind="stable")] = np.arange(a)
        p = np.abs(1.0 / ((y * (rank >= n_sig)[:, None]).sum(axis=0) + EPS))
    elif method == 1:
        p = np.abs((w[:, None] * y).sum(axis=0))
    else:
        wt = w if mutant == "mvdr_weighted_by_w" else 1.0 / w
        p = np.abs(1.0 / ((wt[:, None] * y).sum(axis=0) + EPS))
    with np.errstate(divide="ignore"):
        return 20.0 * np.log10(p / (p.mean() if mutant == "norm_mean" else p.max()))


def deviation(got, ref):
    """Largest |got - ref| in dB over the scan; where the reference lies above -200 dB both sides must be finite (elsewhere equal infinities agree)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    live = ref > -200.0
    assert np.all(np.isfinite(ref[live])) and np.all(np.isfinite(got[live])), "non-finite value where the reference lies above -200 dB"
    same = (got == ref) & ~live
    with np.errstate(invalid="ignore"):
        d = np.where(same, 0.0, np.abs(got - ref))
    return float(np.nan_to_num(d, nan=np.inf).max())


def accept(got, ref, tol):
    try:
        return deviation(got, ref) <= tol
    except AssertionError:
        return False
