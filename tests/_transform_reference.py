"""Plain long-double restatement of the transforms every product of the library passes through, for the tests that compare the
range stage, the Doppler kernels and the OFDM modulator / demodulator value by value (tests/test_transform_reference_cpu.py,
tests/test_gpu_transforms.py):

  * ``dft``: a direct sum (a gathered twiddle matrix times the input), MATLAB's zero-pad-or-truncate ``fft(x, N)`` / ``ifft(x, N)``;
  * ``kaiser(n, 3)``: the I0 power series;
  * ``rdm_plane``: fft2D.m:37-46 in the explicit form of the header of csrc/rdm.hip and of ``oracle.rdm_explicit``;
  * ``ofdm_modulate`` / ``ofdm_demodulate``: oracle/ofdm.py;
  * ``check``: the one comparison rule.

NumPy ``longdouble`` / ``clongdouble`` only (x87 extended precision, eps = 1.08e-19): no FFT library, no fp64 constant on the way.
TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

LD, CLD = np.longdouble, np.clongdouble
assert np.finfo(LD).eps < 1e-18, "tests/_transform_reference.py needs an extended-precision long double"
PI = 4 * np.arctan(LD(1))
EPS64 = float(np.finfo(np.float64).eps)


def _cld(x):
    return np.asarray(x).astype(CLD)


def twiddles(N: int, sign: int) -> np.ndarray:
    """exp(sign 2 pi j m / N), m = 0..N-1; the angle is reduced to the first octant in integers first, so every entry carries one long-double rounding."""
    m = np.arange(N, dtype=np.int64)
    e = 8 * m                                               # angle in units of 2 pi / (8 N); octant = e // N
    octant, r = e // N, e % N                               # angle = (octant + r / N) pi / 4
    odd = (octant % 2) == 1
    r = np.where(odd, N - r, r)                             # odd octants: measure back from the next axis / diagonal
    a = (PI / 4) * r.astype(LD) / LD(N)                     # in [0, pi / 4]
    c, s = np.cos(a), np.sin(a)
    q = ((octant + 1) // 2) % 4                             # the nearest axis: angle = q pi / 2 + sg a
    sg = np.where(odd, LD(-1), LD(1))
    cq = np.array([1, 0, -1, 0], dtype=LD)[q]
    sq = np.array([0, 1, 0, -1], dtype=LD)[q]
    re = cq * c - sq * (sg * s)
    im = sq * c + cq * (sg * s)
    return re + 1j * (LD(sign) * im)


def dft(x: np.ndarray, N: int, sign: int, out_idx=None) -> np.ndarray:
    """sum_n x[n] exp(sign 2 pi j k n / N) over the first min(len(x), N) inputs (MATLAB zero-pads or truncates to N), along axis 0, for the outputs k in
    ``out_idx`` (all N when None).  Unscaled."""
    x = _cld(x)
    m = min(x.shape[0], N)
    k = np.arange(N, dtype=np.int64) if out_idx is None else np.asarray(out_idx, dtype=np.int64)
    ph = (k[:, None] * np.arange(m, dtype=np.int64)[None, :]) % N
    w = twiddles(N, sign)[ph]
    return (w @ x[:m].reshape(m, -1)).reshape((k.size,) + x.shape[1:])


def _bessel_i0(x: np.ndarray) -> np.ndarray:
    q = (x.astype(LD) / 2) ** 2
    term = np.ones_like(q)
    total = np.ones_like(q)
    for k in range(1, 200):
        term = term * q / (LD(k) * LD(k))
        total = total + term
        if np.all(term < LD(1e-22) * total):
            break
    return total


_KAISER = {}


def kaiser(n: int, beta=3) -> np.ndarray:
    """Signal Processing Toolbox ``kaiser(n, beta)``: w[k] = I0(beta sqrt(1 - ((2 k - (n - 1)) / (n - 1))^2)) / I0(beta), for odd and even n alike
    (1 - t^2 = 4 k (n - 1 - k) / (n - 1)^2 in integers).  One window per length is kept."""
    key = (int(n), beta)
    if key not in _KAISER:
        if n == 1:
            w = np.ones(1, dtype=LD)
        else:
            k = np.arange(n, dtype=np.int64)
            arg = (4 * k * (n - 1 - k)).astype(LD) / LD((n - 1) * (n - 1))
            w = _bessel_i0(LD(beta) * np.sqrt(arg)) / _bessel_i0(np.array([beta], dtype=LD))[0]
        w.setflags(write=False)
        _KAISER[key] = w
    return _KAISER[key]


def fftshift_index(n: int) -> np.ndarray:
    """fftshift(x) = x[fftshift_index(n)]: out[i] = in[(i + ceil(n / 2)) mod n]."""
    return (np.arange(n) + (n + 1) // 2) % n


def rdm_plane(rx: np.ndarray, tx: np.ndarray, n_ifft: int, n_fft: int, rows=None, l_shift=None) -> np.ndarray:
    """Rows ``rows`` (all when None) of one antenna plane of the range-Doppler map, [len(rows) x n_fft], from rx, tx [K x L] (fft2D.m:37-46).
    ``l_shift``: the slow-time rotation, floor(L / 2) of ifftshift unless a test asks for a wrong one."""
    rx, tx = _cld(rx), _cld(tx)
    K, L = rx.shape
    rows = np.arange(n_ifft) if rows is None else np.asarray(rows, dtype=np.int64)
    c = rx * np.conj(tx)                                                   # 1  fft2D.m:37
    c = c * kaiser(K, 3)[:, None]                                          # 2  :43
    r = dft(c, n_ifft, +1, rows) * (np.sqrt(LD(n_ifft)) / LD(n_ifft))      # 3  :44 ifft(., nIFFT, 1) * sqrt(nIFFT)
    r = r * kaiser(n_ifft, 3)[fftshift_index(n_ifft)][rows][:, None]       # 4  :45 under the all-dimension shifts of :44 and :46
    half = L // 2 if l_shift is None else int(l_shift)
    r = r[:, (np.arange(L) + half) % L]                                    # 5  :44 ifftshift over the whole of L: out[i] = in[(i + floor(L / 2)) mod L]
    d = dft(r.T, n_fft, -1).T / np.sqrt(LD(n_fft))                         # 6  :46 fft(., nFFT, 2) / sqrt(nFFT): zero-pads or truncates L
    return d[:, fftshift_index(n_fft)]                                     # 7  :46 fftshift


def cp_terms(nfft: int, scs_khz: int):
    """(144 s, 16 s 2^mu, mu) with s = Nfft / 2048 as exact fractions (numerator, denominator): TS 38.211 5.3.1 scaled to Nfft."""
    from fractions import Fraction
    mu = {15: 0, 30: 1, 60: 2, 120: 3}[int(scs_khz)]
    s = Fraction(nfft, 2048)
    return 144 * s, 16 * s * 2 ** mu, mu


def cp_lengths(nfft: int, scs_khz: int, n_symbols: int, first_symbol: int = 0) -> np.ndarray:
    base, extra, mu = cp_terms(nfft, scs_khz)
    assert base.denominator == 1 and extra.denominator == 1, f"no integral cyclic prefix at Nfft = {nfft}: {base}, {extra}"    # no rounding
    l = first_symbol + np.arange(n_symbols)
    return np.where(l % (7 * 2 ** mu) == 0, int(base) + int(extra), int(base)).astype(np.int64)


def symbol_starts(nfft, scs_khz, n_symbols, first_symbol=0):
    cps = cp_lengths(nfft, scs_khz, n_symbols, first_symbol)
    return np.concatenate([[0], np.cumsum(cps + nfft)[:-1]]).astype(np.int64), cps


def raised_cosine_edge(n_w: int) -> np.ndarray:
    i = np.arange(1, n_w + 1).astype(LD)
    return (1 - np.sin(PI * (n_w + 1 - 2 * i) / (2 * n_w))) / 2


def ofdm_modulate(grid: np.ndarray, nfft: int, scs_khz: int, windowing: int = 0, first_symbol: int = 0, td_idx=None) -> np.ndarray:
    """grid [K x L x A] -> waveform [T x A] (oracle/ofdm.py ofdm_modulate).  ``td_idx``: the samples of each symbol's useful part to evaluate; the
    waveform samples made of any other one are NaN."""
    grid = _cld(grid)
    k, l, a = grid.shape
    starts, cps = symbol_starts(nfft, scs_khz, l, first_symbol)
    total = int(starts[-1] + cps[-1] + nfft)
    first = (nfft - k) // 2
    kbin = np.arange(k) + first - nfft // 2                                # signed bin of each grid row
    idx = np.arange(nfft) if td_idx is None else np.asarray(td_idx, dtype=np.int64)
    ph = (idx[:, None] * (kbin % nfft)[None, :]) % nfft
    td = np.full((nfft, l, a), np.nan, dtype=CLD)
    td[idx] = (twiddles(nfft, +1)[ph] @ grid.reshape(k, l * a)).reshape(idx.size, l, a) / LD(nfft)
    wave = np.zeros((total, a), dtype=CLD)
    for s in range(l):
        cp, o = int(cps[s]), int(starts[s])
        wave[o:o + cp] = td[nfft - cp:, s, :]
        wave[o + cp:o + cp + nfft] = td[:, s, :]
    n_w = int(windowing)
    if n_w > 0:
        assert n_w <= int(cps.min())
        rise = raised_cosine_edge(n_w)[:, None]
        fall = rise[::-1]
        for s in range(l):
            nxt = (s + 1) % l
            cpn = int(cps[nxt])
            e = int(starts[s]) + int(cps[s]) + nfft
            wave[e - n_w:e] = fall * wave[e - n_w:e] + rise * td[nfft - cpn - n_w:nfft - cpn, nxt, :]
    return wave


def ofdm_demodulate(wave: np.ndarray, n_sc: int, nfft: int, scs_khz: int, rows=None, cp_offset=None) -> np.ndarray:
    """waveform [T x R] -> rows ``rows`` (all when None) of the grid [n_sc x L x R] of the whole symbols in T (oracle/ofdm.py ofdm_demodulate).
    ``cp_offset``: the window's start inside a CP of length cp, fix(cp / 2) unless a test asks for a wrong one."""
    wave = _cld(wave)
    t, r = wave.shape
    starts, cps = symbol_starts(nfft, scs_khz, int(t // nfft) + 1)
    l = int(np.searchsorted(starts + cps + nfft, t, side="right"))
    assert l > 0
    rows = np.arange(n_sc) if rows is None else np.asarray(rows, dtype=np.int64)
    kbin = rows + (nfft - n_sc) // 2 - nfft // 2
    out = np.empty((rows.size, l, r), dtype=CLD)
    tw = twiddles(nfft, +1)
    for s in range(l):
        cp = int(cps[s])
        off = cp // 2 if cp_offset is None else int(cp_offset(cp))         # fix(cp / 2)
        w0 = int(starts[s]) + off
        x = dft(wave[w0:w0 + nfft], nfft, -1, kbin % nfft)
        out[:, s, :] = x * tw[(kbin * (cp - off)) % nfft][:, None]         # exp(+2 pi j kb (cp - fix(cp / 2)) / Nfft)
    return out


# ---------------------------------------------------------------- the comparison rule
MARGIN = 32


def measure(got, ref, oracle64) -> SimpleNamespace:
    """The figures of ``check``: rms of the reference, e_ref = max |oracle64 - ref| (the project's own fp64 oracle against the long-double reference on the
    same input: neither is code under test), floor = 4 eps64 rms (one stored fp64 value of the largest magnitude that occurs, about 4 rms for these
    inputs, carries that much rounding), tol = 32 max(e_ref, floor), err = max |got - ref| and the index of its element."""
    ref = np.asarray(ref)
    kind = CLD if np.iscomplexobj(ref) else LD
    ref = ref.astype(kind)
    got, oracle64 = np.asarray(got), np.asarray(oracle64)
    assert got.shape == ref.shape == oracle64.shape, (got.shape, ref.shape, oracle64.shape)
    rms = float(np.sqrt(np.mean(np.abs(ref) ** 2)))
    e_ref = float(np.abs(oracle64.astype(kind) - ref).max())
    d = np.abs(got.astype(kind) - ref)
    d = np.where(np.isfinite(d), d, np.inf)                                # a NaN in the result is the worst element, not a pass
    idx = np.unravel_index(int(np.argmax(d)), d.shape)
    floor = 4 * EPS64 * rms
    return SimpleNamespace(rms=rms, e_ref=e_ref, floor=floor, tol=MARGIN * max(e_ref, floor), err=float(d[idx]), idx=tuple(int(i) for i in idx),
                           peak=float(np.abs(ref).max()))


def check(got, ref, oracle64, report=None):
    """Assert max |got - ref| <= tol element by element, and tol <= 1e-10 rms (the project's stated tolerance: a broken oracle cannot widen the test).
    Returns the index of the worst element; ``report`` (optional) receives the figures first."""
    m = measure(got, ref, oracle64)
    if report is not None:
        report(m)
    assert m.tol <= 1e-10 * m.rms, f"the fp64 oracle is {m.e_ref / m.rms:.3e} rms away from the long-double reference: tolerance {m.tol / m.rms:.3e} rms exceeds 1e-10"
    assert m.err <= m.tol, (f"worst element {m.idx}: |got - ref| = {m.err / m.rms:.3e} rms > tol = {m.tol / m.rms:.3e} rms "
                            f"(e_ref = {m.e_ref / m.rms:.3e} rms, ratio {m.err / max(m.e_ref, 1e-300):.1f})")
    return m.idx


def edge_rows(n: int, n_random: int, seed: int) -> np.ndarray:
    """Row subset for the 2048- and 4096-point cases: row 0, row n - 1, both sides of every 512-row boundary and seeded random rows."""
    fixed = {0, n - 1}
    for b in range(512, n, 512):
        fixed |= {b - 1, b}
    rng = np.random.default_rng(seed)
    extra = rng.choice(n, size=n_random, replace=False)
    return np.array(sorted(fixed | set(int(i) for i in extra)), dtype=np.int64)


# ---------------------------------------------------------------- the shapes both test files run, and their inputs
# (a) the full plane: K, nIFFT, L, nFFT, A, ant, zeroed tx symbols, rows checked (None: all)
PLANE_CASES = [
    dict(K=48, n_ifft=64, L=7, n_fft=16, A=1, ant=0, zero=None, subset=False),       # smallest dispatch; odd L; zero padding on both axes
    dict(K=49, n_ifft=64, L=14, n_fft=8, A=2, ant=1, zero=None, subset=False),       # odd K; L > nFFT truncation; plane offset K L ant
    dict(K=128, n_ifft=128, L=28, n_fft=64, A=3, ant=2, zero=None, subset=False),    # K == nIFFT
    dict(K=200, n_ifft=256, L=13, n_fft=32, A=1, ant=0, zero=None, subset=False),    # FftStockham<256>, PER == 1
    dict(K=288, n_ifft=512, L=56, n_fft=32, A=2, ant=1, zero=(14, 28), subset=False),  # truncation at even L; zero-column early exit
    dict(K=612, n_ifft=1024, L=20, n_fft=128, A=1, ant=0, zero=None, subset=False),
    dict(K=1596, n_ifft=2048, L=13, n_fft=512, A=1, ant=0, zero=None, subset=True),
    dict(K=3276, n_ifft=4096, L=28, n_fft=256, A=3, ant=2, zero=(14, 28), subset=True),   # Fft4096W full drain
    dict(K=4096, n_ifft=4096, L=9, n_fft=16, A=1, ant=0, zero=None, subset=True),    # K == nIFFT at the hot size
]
# (b) the power window of fft2D: CUT rectangle (1-based, inclusive) and the planted tone's 0-based (row, Doppler bin); guard (2, 2), training (1, 1)
WINDOW_CASES = [
    dict(n_ifft=4096, K=1200, n_fft=256, L=28, A=3, rows=(2600, 2700), cols=(170, 210), r0=2650, d0=64),    # dft8_one path + fft256, zero-padded
    dict(n_ifft=4096, K=1200, n_fft=256, L=270, A=3, rows=(1000, 1050), cols=(110, 150), r0=1024, d0=0),    # full last pass + fft256 truncating
    dict(n_ifft=128, K=100, n_fft=256, L=256, A=4, rows=(40, 76), cols=(110, 150), r0=57, d0=5),            # fft256 with L == nFFT
    dict(n_ifft=512, K=288, n_fft=64, L=28, A=3, rows=(200, 236), cols=(10, 55), r0=217, d0=16),            # generic Doppler kernel, zero-padded
    dict(n_ifft=64, K=48, n_fft=16, L=28, A=4, rows=(4, 61), cols=(4, 13), r0=30, d0=0),                    # generic kernel truncating; window = the map
    dict(n_ifft=256, K=200, n_fft=512, L=300, A=3, rows=(100, 119), cols=(330, 430), r0=109, d0=128),       # generic kernel at a large nFFT
]
GUARD, TRAIN, PFA = (2, 2), (1, 1), 1e-9          # sensing.detection.cfar2D's detector; radar.m:15
# (c) OFDM: n_sc, Nfft, SCS, L, A
OFDM_CASES = [
    dict(n_sc=72, nfft=128, scs=15, L=15, A=2),      # odd CPs 9 / 10; long CP at l = 0, 7, 14
    dict(n_sc=128, nfft=128, scs=30, L=29, A=1),     # n_sc == Nfft; CP 9 / 11
    dict(n_sc=2, nfft=128, scs=120, L=57, A=1),      # smallest n_sc; long CP 17 at l = 0 and l = 56
    dict(n_sc=180, nfft=256, scs=60, L=30, A=3),     # FftStockham<256>; period 28
    dict(n_sc=624, nfft=1024, scs=60, L=29, A=1),    # demodulator away from 30 kHz
    dict(n_sc=3276, nfft=4096, scs=15, L=15, A=2),   # Fft4096, dshift 144 / 160
    dict(n_sc=3276, nfft=4096, scs=120, L=57, A=1),  # Fft4096, dshift 144 / 272, l = 56
]
WINDOWED_CASES = [
    dict(n_sc=72, nfft=128, scs=15, L=15, A=2, n_slot=0, windowing=4),
    dict(n_sc=180, nfft=256, scs=60, L=30, A=3, n_slot=2, windowing=8),
]


def case_id(c) -> str:
    return "-".join(str(c[k]) for k in ("K", "n_sc", "n_ifft", "nfft", "scs", "L", "n_fft", "n_slot") if k in c)


def qpsk(rng, shape) -> np.ndarray:
    return np.asfortranarray(((rng.integers(0, 2, shape) * 2 - 1) + 1j * (rng.integers(0, 2, shape) * 2 - 1)) / np.sqrt(2.0))


def cnormal(rng, shape) -> np.ndarray:
    """Complex normal, unit variance."""
    return np.asfortranarray((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2.0))


def plane_inputs(c, seed=11):
    """(rx, tx) [K x L x A]: noise-like rx, unit-modulus QPSK tx with the case's symbol columns zeroed."""
    rng = np.random.default_rng([seed, c["K"], c["L"], c["n_fft"]])
    shape = (c["K"], c["L"], c["A"])
    rx, tx = cnormal(rng, shape), qpsk(rng, shape)
    if c["zero"]:
        tx[:, c["zero"][0]:c["zero"][1], :] = 0
    return rx, tx


def plane_rows(c) -> np.ndarray:
    return edge_rows(c["n_ifft"], 90, c["K"]) if c["subset"] else np.arange(c["n_ifft"])


def tone_amplitude(c, over=50.0) -> float:
    """The amplitude at which the planted tone's cell stands `over` times above the map's noise floor: its coherent gain through both transforms is
    (sum w)^2 Lu / sum w^2 over unit-variance noise, w = kaiser(K, 3), Lu = min(L, nFFT) slow-time samples used."""
    w = kaiser(c["K"], 3)
    gain = float(w.sum() ** 2 / (w * w).sum()) * min(c["L"], c["n_fft"])
    return float(np.sqrt(over / gain))


def window_inputs(c, seed=23):
    """(rx, tx, amp, the tone's energy over the noise grid's): the grids of a power-window case, one tone amp tx[k, l] exp(-2 pi j k r0 / nIFFT)
    exp(+2 pi j l d0 / nFFT) added to every antenna plane of rx."""
    rng = np.random.default_rng([seed, c["K"], c["L"], c["n_fft"]])
    shape = (c["K"], c["L"], c["A"])
    rx, tx = cnormal(rng, shape), qpsk(rng, shape)
    amp = tone_amplitude(c)
    k, l = np.arange(c["K"])[:, None, None], np.arange(c["L"])[None, :, None]
    tone = amp * tx * np.exp(-2j * np.pi * ((k * c["r0"]) % c["n_ifft"]) / c["n_ifft"]) * np.exp(2j * np.pi * ((l * c["d0"]) % c["n_fft"]) / c["n_fft"])
    return np.asfortranarray(rx + tone), tx, amp, float(np.sum(np.abs(tone) ** 2) / np.sum(np.abs(rx) ** 2))


def window_geometry(c):
    """0-based (first row, rows, first column, columns) of the power window: the CUT rectangle +- (guard + training)."""
    hr, hc = GUARD[0] + TRAIN[0], GUARD[1] + TRAIN[1]
    r_lo, c_lo = c["rows"][0] - 1 - hr, c["cols"][0] - 1 - hc
    return r_lo, c["rows"][1] - c["rows"][0] + 1 + 2 * hr, c_lo, c["cols"][1] - c["cols"][0] + 1 + 2 * hc


def ofdm_inputs(c, seed=37, first_symbol=0):
    """(grid [n_sc x L x A] QPSK, noise-like waveform [T x A] of exactly L symbols)."""
    rng = np.random.default_rng([seed, c["n_sc"], c["nfft"], c["scs"]])
    grid = qpsk(rng, (c["n_sc"], c["L"], c["A"]))
    starts, cps = symbol_starts(c["nfft"], c["scs"], c["L"], first_symbol)
    t = int(starts[-1] + cps[-1] + c["nfft"])
    return grid, cnormal(rng, (t, c["A"]))


def ofdm_subsets(c):
    """(useful-part samples, grid rows) a case is checked at: everything below 4096 points; there the first and last samples, both sides of the places where
    each CP length begins inside the useful part, the grid's edge and centre rows, and seeded random ones -- about 100 each."""
    nfft, n_sc = c["nfft"], c["n_sc"]
    if nfft < 4096:
        return None, None
    rng = np.random.default_rng([5, n_sc, c["scs"]])
    cps = set(int(v) for v in cp_lengths(nfft, c["scs"], c["L"]))
    td = {0, 1, nfft - 1, nfft // 2}
    for cp in cps:
        td |= {nfft - cp - 1, nfft - cp, nfft - cp + 1}
    td |= set(int(i) for i in rng.choice(nfft, 90, replace=False))
    rows = {0, 1, n_sc // 2 - 1, n_sc // 2, n_sc - 2, n_sc - 1} | set(int(i) for i in rng.choice(n_sc, 90, replace=False))
    return np.array(sorted(td)), np.array(sorted(rows))
