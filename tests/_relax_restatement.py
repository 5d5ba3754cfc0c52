"""NumPy restatement of isac_fft2d_relax_targets (include/isac_relax.h, DESIGN.md section 5 -- project-defined): the joint re-fit (RELAX) of Doppler tones on range rows
[nr x L x A], every bracket decision with its margin, the cluster schedule, and the scenes its tests share.

Every sum over the symbols and the sign of P' run in np.longdouble; R, the amplitudes C and nu are rounded to fp64 where the device stores them (once per re-fit of a
row, once per search).  The margin of a bracket decision is min(|d(nu - h)|, |d(nu + h)|), d = sum_a Im(conj(X_a) D_a), each relative to sum_a |X_a| |D_a| at the same
frequency: the size of the terms whose cancellation forms d, and so the scale of its rounding error (about L 2^-53 of it).  An all-zero row has no scale: its decision
is forced (d = 0) and its margin is infinite."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import oracle as O

import _clean_restatement as K
import _refine_restatement as R
import _target_list_restatement as T

_LD = np.longdouble
_PI_LD = 4 * np.arctan(_LD(1))
N_BISECT = 40
CYCLES, SPAN_ROWS, BOX = 16, 2, 0.5


def _phasor(nu, L, active):
    """p_nu [L] in long double: e^{-2 pi j nu l} on the active symbols, 0 on the others."""
    ph = (-2 * _PI_LD * _LD(nu)) * np.arange(L).astype(_LD)
    return np.where(active, np.cos(ph) + 1j * np.sin(ph), 0).astype(np.clongdouble)


def _dp(z, l_ld, nu, active):
    """(d, scale) of P'(nu) on the row z [L x A] (long double): d = sum_a Im(conj(X_a) D_a), scale = sum_a |X_a| |D_a|."""
    zp = z * _phasor(nu, z.shape[0], active)[:, None]
    x, d = zp.sum(axis=0), (zp * l_ld[:, None]).sum(axis=0)
    return (x.real * d.imag - x.imag * d.real).sum(), (np.abs(x) * np.abs(d)).sum()


def spans(wr, n_rows, span_rows):
    """(lo, hi) of every entry's span, 0-based window rows, clipped to the window."""
    return [(max(int(r) - span_rows, 0), min(int(r) + span_rows, n_rows - 1)) for r in wr]


def clusters(wr, n_rows, span_rows):
    """Entries whose spans share a row, transitively: a list of index lists, each in input order, ordered by their first entry."""
    sp = spans(wr, n_rows, span_rows)
    label = list(range(len(sp)))
    moved = True
    while moved:
        moved = False
        for i, (a0, a1) in enumerate(sp):
            for k, (b0, b1) in enumerate(sp):
                if a0 <= b1 and b0 <= a1 and label[k] < label[i]:
                    label[i], moved = label[k], True
    out = {}
    for i, c in enumerate(label):
        out.setdefault(c, []).append(i)
    return [out[c] for c in sorted(out)]


def order(wr, n_rows, span_rows, schedule):
    """The entries of one sweep in the order they are served: 'sequential' = input order; 'cluster' = the device's: position k of every cluster, k = 0, 1, ..."""
    if schedule == "sequential":
        return list(range(len(wr)))
    cl = clusters(wr, n_rows, span_rows)
    return [c[k] for k in range(max(map(len, cl), default=0)) for c in cl if k < len(c)]


def relax(rows, wr, nu_in, n_fft, cycles=CYCLES, span_rows=SPAN_ROWS, box=BOX, sym_active=None, schedule="sequential"):
    """The call on rows [nr x L x A] for the entries (wr [n] 0-based window rows, nu_in [n]).  Returns nu, status, shift, last_step, power, snapshots [A x n], residual,
    C (list of [span x A]), ``decisions`` [cycles x n] (True: the bracket held), ``margins`` [cycles x n] and ``energy`` [cycles + 1] (sum |R|^2 after step 0 and after
    every cycle)."""
    Rr = np.array(rows, dtype=np.complex128)
    nr, L, A = Rr.shape
    wr, nu_in = np.asarray(wr, dtype=np.int64), np.asarray(nu_in, dtype=np.float64)
    n = wr.size
    active = np.ones(L, dtype=bool) if sym_active is None else np.asarray(sym_active).astype(bool)
    if not active.any():
        raise ValueError("no active symbol")
    n_act = _LD(int(active.sum()))
    l_ld = np.arange(L).astype(_LD)
    sp = spans(wr, nr, span_rows)
    C = [np.zeros((hi - lo + 1, A), dtype=np.complex128) for lo, hi in sp]
    nu, prev = nu_in.copy(), nu_in.copy()
    h = box / float(L)

    def refit(j, nu_old, nu_new):
        p_old, p_new = _phasor(nu_old, L, active), _phasor(nu_new, L, active)
        lo, hi = sp[j]
        for q, r in enumerate(range(lo, hi + 1)):
            z = Rr[r].astype(np.clongdouble) + C[j][q].astype(np.clongdouble)[None, :] * np.conj(p_old)[:, None]
            c_new = ((z * p_new[:, None]).sum(axis=0) / n_act).astype(np.complex128)
            out = z - c_new.astype(np.clongdouble)[None, :] * np.conj(p_new)[:, None]
            Rr[r][active] = out[active].astype(np.complex128)
            C[j][q] = c_new

    sweep = order(wr, nr, span_rows, schedule)
    for j in sweep:                                                        # step 0
        refit(j, nu[j], nu[j])
    energy = [float((np.abs(Rr) ** 2).sum())]
    decisions, margins = np.zeros((cycles, n), dtype=bool), np.full((cycles, n), np.inf)
    for cyc in range(cycles):
        for j in sweep:
            q = int(wr[j]) - sp[j][0]
            z = Rr[wr[j]].astype(np.clongdouble) + C[j][q].astype(np.clongdouble)[None, :] * np.conj(_phasor(nu[j], L, active))[:, None]
            a, b = nu[j] - h, nu[j] + h                                    # (fp64, as the device forms them)
            (d_lo, s_lo), (d_hi, s_hi) = _dp(z, l_ld, a, active), _dp(z, l_ld, b, active)
            ok = bool(d_lo > 0 and d_hi < 0)
            decisions[cyc, j] = ok
            if s_lo > 0 and s_hi > 0:
                margins[cyc, j] = float(min(abs(d_lo) / s_lo, abs(d_hi) / s_hi))
            new = nu[j]
            if ok:
                a, b = _LD(a), _LD(b)
                for _ in range(N_BISECT):
                    mid = (a + b) / 2
                    if _dp(z, l_ld, mid, active)[0] > 0:
                        a = mid
                    else:
                        b = mid
                new = float((a + b) / 2)
            refit(j, nu[j], new)
            prev[j], nu[j] = nu[j], new
        energy.append(float((np.abs(Rr) ** 2).sum()))
    s = np.stack([float(n_act) * C[j][int(wr[j]) - sp[j][0]] for j in range(n)], axis=1) if n else np.zeros((A, 0), dtype=np.complex128)
    power = np.array([sum(x.real * x.real + x.imag * x.imag for x in s[:, j]) / n_fft for j in range(n)], dtype=np.float64)
    return SimpleNamespace(nu=nu, status=(~decisions[-1]).astype(np.int64) if cycles else np.zeros(n, dtype=np.int64), shift=np.abs(nu - nu_in) * L,
                           last_step=np.abs(nu - prev) * L, power=power, snapshots=s / np.sqrt(float(n_fft)), residual=Rr, C=C, decisions=decisions, margins=margins,
                           energy=np.array(energy))


# ---------------------------------------------------------------- exact tones (the truth-recovery scenes of tests/test_relax_cpu.py)
def tone_rows(L, nus, amps, A=4, seed=5):
    """One row [1 x L x A] of exact tones sum_q amps[q] s_q[a] e^{+2 pi j nus[q] l} with random unit-modulus steering s_q, no noise."""
    rng = np.random.default_rng(seed)
    l = np.arange(L)
    y = np.zeros((L, A), dtype=np.complex128)
    for v, amp in zip(nus, amps):
        y += amp * np.exp(2j * np.pi * v * l)[:, None] * np.exp(2j * np.pi * rng.random(A))[None, :]
    return y[None]


def sequential(rows, wr, nu_near, n_fft, span_rows=0, box=BOX):
    """One tone after another, each estimated once while the later ones are still in the data (the order of isac_fft2d_clean_targets): the maximum of the periodogram
    within box / L of nu_near[i], then the subtraction.  Returns the estimates."""
    Rr, out = np.array(rows, dtype=np.complex128), []
    for r, v in zip(wr, nu_near):
        one = relax(Rr, [r], [v], n_fft, cycles=1, span_rows=span_rows, box=box)
        assert one.status[0] == 0
        out.append(float(one.nu[0]))
        Rr = one.residual
    return np.array(out)


# ---------------------------------------------------------------- the scenes of tests/test_gpu_relax.py (conditioning: tests/test_relax_cpu.py)
# All at 24 PRB (K = 288, nIFFT = 512).  Two targets at ONE range (105.9 m: row 12 of the map) whose tones lie 1.5 lobes apart, echo amplitudes 1 : 0.5.  ``v``: the
# velocities, +- 0.75 lobes (nu = v / (nFFT vRes), a lobe = 1 / L); ``slots``: numSlots of radarParams (nFFT); ``cut``: the grid is cut to that many symbols (29: a
# short last quarter).
_AT_ONE_RANGE = ((100.0, 20.0, 1.5), (100.0, -20.0, 1.5))
RCS = (1.0, 0.25)
TARGET_ROW = 12


def _scene(n_ants, n_slots, slots, lobes=0.75, seed=61, cut=None, upa=None, zero_s=False):
    return dict(n_ants=n_ants, n_slots=n_slots, slots=slots, lobes=lobes, seed=seed, cut=cut, upa=upa, zero_s=zero_s)


SCENES = {
    "a4_L28": _scene(4, 2, 6),
    "a1_L29": _scene(1, 3, 6, seed=62, cut=29),
    "a65_L28": _scene(65, 2, 6, seed=63),                                  # more antennas than the 64 quads of a workgroup: the evaluation's second pass
    "a4_L280": _scene(4, 20, 20, seed=64),                                 # more symbols than threads
    "upa2x2_L28": _scene(4, 2, 6, seed=65, upa=(2, 2)),
    "a4_L56_gap": _scene(4, 4, 6, seed=66, zero_s=True),                   # the 'S' slot (symbols 42 .. 55) silent
}
# "a4_L28" once more (another seed) at the asymmetric guard / training bands T.READER_BANDS: the rows the context holds are the CUT rows +- hr = 4, not 3, and every row
# index of the call (the entries' rows, the spans, the edge rows) is taken against that window
BANDS_SCENE = "a4_L28_g13_t32"
SCENES[BANDS_SCENE] = _scene(4, 2, 6, seed=67)
T.BANDS[BANDS_SCENE] = T.READER_BANDS
GAP_MASK = K.GAP_MASK
# ... and the end-to-end scene of tests/test_relax_cpu.py (oracle only): 16 elements, the tones 1.8 lobes apart
OTHER = {"e2e_a16": _scene(16, 2, 6, lobes=0.9, seed=71)}


def is_upa(scene):
    return SCENES[scene]["upa"] is not None


def n_symbols(scene):
    s = {**SCENES, **OTHER}[scene]
    return s["cut"] or 14 * s["n_slots"]


@functools.lru_cache(maxsize=None)
def make(scene):
    """The scene (conftest.make_scene's namespace, sc.rp the oracle's radarParams for it).  Shared: callers must not modify it."""
    from conftest import make_scene
    s = {**SCENES, **OTHER}[scene]
    L = n_symbols(scene)
    probe = make_scene(n_ants=1, n_slots=1, nrb=24, num_slots_param=s["slots"], with_noise=False)
    lobe = float(probe.rp.nFFT) * float(probe.rp.vRes) / L                 # one lobe (1 / L in nu) as a velocity
    sc = make_scene(n_ants=s["n_ants"], n_slots=s["n_slots"], nrb=24, num_slots_param=s["slots"], seed=s["seed"], targets=_AT_ONE_RANGE,
                    velocity=(s["lobes"] * lobe, -s["lobes"] * lobe), zero_s_slots=s["zero_s"])
    sc.cell.rcs = np.asarray(RCS, dtype=np.float64)
    if s["upa"]:
        sc.cell.gNBSenAntenna = SimpleNamespace(kind="upa", nV=s["upa"][0], nH=s["upa"][1], dV=0.5, dH=0.5)
        sc.nV, sc.nH = s["upa"]
    sc.rp = O.radar_params(sc.cell, sc.carrier, sc.wave)
    if s["cut"]:                                                           # the first `cut` symbols of the grid and of the waveform
        starts, _ = O.symbol_starts(sc.wave.Nfft, 30, L + 1)
        t = int(starts[L])
        sc.tx_grid, sc.tx_wave, sc.noise = np.asfortranarray(sc.tx_grid[:, :L]), np.asfortranarray(sc.tx_wave[:t]), np.asfortranarray(sc.noise[:t])
        sc.L, sc.T = L, t
    return sc


def true_nu(sc):
    return np.array([float(t["Velocity"]) for t in sc.rp.targetRealPos]) / (float(sc.rp.nFFT) * float(sc.rp.vRes))


@functools.lru_cache(maxsize=None)
def oracle_rows(scene):
    """Oracle only: O.mono_static_sensing -> the window's range rows and the geometry (tests/_clean_restatement.py: geometry).  Shared; callers must not modify it."""
    sc = make(scene)
    rp = sc.rp
    g = K.geometry(rp, T.oracle_config(scene, rp))                         # the default bands for every scene but BANDS_SCENE
    echo = O.mono_static_sensing(sc.tx_wave, sc.tx_grid.shape, sc.carrier, rp, sc.los, sc.noise, nfft=sc.wave.Nfft)
    rows = R.range_rows(echo, sc.tx_grid, g.n_ifft)[g.first_row - 1:g.first_row - 1 + g.n_rows].copy()
    return SimpleNamespace(sc=sc, rp=rp, g=g, rows=rows, L=rows.shape[1], nu=true_nu(sc))


def _pair(sc, d0=0.05, d1=-0.03, dr=0):
    """The two tones on the targets' row (the second ``dr`` rows away), d0 / L and d1 / L off the truth -- about where a sequential estimate lands."""
    nu = true_nu(sc)
    return [TARGET_ROW, TARGET_ROW + dr], [nu[0] + d0 / sc.L, nu[1] + d1 / sc.L]


def _many(sc, g):
    """64 entries: 16 frequencies 1.4 lobes apart on each of the rows 11 .. 14, 0.35 lobes further from row to row -- one cluster; the targets' two tones first."""
    row, nu = _pair(sc)
    for r in range(TARGET_ROW - 1, TARGET_ROW + 3):
        for k in range(16):
            v = (k - 7.5) * 1.4 / sc.L + 0.35 * (r - TARGET_ROW) / sc.L
            if len(row) < 64 and not (r == TARGET_ROW and min(abs(v - x) for x in nu[:2]) * sc.L < 0.7):
                row.append(r)
                nu.append(v)
    assert len(row) == 64
    return row, nu


def _three_clusters(sc, g):
    """The pair, a tone 9 rows away and one on the last CUT row: spans of 5 rows that do not meet; given interleaved."""
    row, nu = _pair(sc)
    return [row[0], TARGET_ROW + 9, g.rect[1], row[1], TARGET_ROW + 10], [nu[0], 0.3 / sc.L, -1.1 / sc.L, nu[1], 1.9 / sc.L]


# name -> (scene, entries(sc, g) -> (row 1-based, nu_in), keywords of ``relax``)
CASES = {
    "one": ("a4_L28", lambda sc, g: ([TARGET_ROW], [true_nu(sc)[0] + 0.05 / sc.L]), {}),
    "pair": ("a4_L28", lambda sc, g: _pair(sc), {}),
    "pair_cycles0": ("a4_L28", lambda sc, g: _pair(sc), dict(cycles=0)),
    "pair_cycles1_span0": ("a4_L28", lambda sc, g: _pair(sc), dict(cycles=1, span_rows=0)),
    "pair_box2": ("a4_L28", lambda sc, g: _pair(sc, 0.4, -0.5), dict(box=2.0, cycles=4)),
    "adjacent_rows": ("a4_L28", lambda sc, g: _pair(sc, dr=1), {}),
    "three_clusters": ("a4_L28", _three_clusters, {}),
    "sixty_four": ("a4_L28", _many, {}),
    "edge_rows": ("a4_L28", lambda sc, g: ([g.rect[0], g.rect[1], TARGET_ROW], [0.4 / sc.L, -0.2 / sc.L, true_nu(sc)[0]]), dict(span_rows=3)),
    "wide_span": ("a4_L28", lambda sc, g: _pair(sc), dict(span_rows=2 ** 31 - 1, cycles=2)),   # every row of the window
    "off_the_lobe": ("a4_L28", lambda sc, g: ([TARGET_ROW], [true_nu(sc)[0] + 0.8 / sc.L]), dict(cycles=3)),   # 0.8 lobes above the only fitted tone: P' < 0 at both ends, status 1
    "a1_L29": ("a1_L29", lambda sc, g: _pair(sc), {}),
    "a65_L28": ("a65_L28", lambda sc, g: _pair(sc), dict(cycles=4)),
    "a4_L280": ("a4_L280", lambda sc, g: _pair(sc), dict(cycles=4)),
    "upa2x2": ("upa2x2_L28", lambda sc, g: _pair(sc), {}),
    "gap_mask": ("a4_L56_gap", lambda sc, g: _pair(sc), dict(sym_active=GAP_MASK)),
    "gap_nomask": ("a4_L56_gap", lambda sc, g: _pair(sc), dict(cycles=4)),
    "bands_pair": (BANDS_SCENE, lambda sc, g: _pair(sc), {}),
    "bands_three_clusters": (BANDS_SCENE, _three_clusters, {}),
    "bands_edge_rows": (BANDS_SCENE, lambda sc, g: ([g.rect[0], g.rect[1], TARGET_ROW], [0.4 / sc.L, -0.2 / sc.L, true_nu(sc)[0]]), dict(span_rows=4)),   # spans that end on the window's first and last row
}


def entries(case):
    """(row [n] 1-based, nu_in [n]) of a case."""
    scene, fn, _ = CASES[case]
    s = oracle_rows(scene)
    row, nu = fn(s.sc, s.g)
    return np.asarray(row, dtype=np.int32), np.asarray(nu, dtype=np.float64)


def run(case, rows, **over):
    """The restatement of a case on rows [nr x L x A] (the oracle's, or a device's)."""
    scene, _, kw = CASES[case]
    s = oracle_rows(scene)
    row, nu = entries(case)
    return relax(rows, row - s.g.first_row, nu, s.g.n_fft, **{**kw, **over})


@functools.lru_cache(maxsize=None)
def oracle_relax(case):
    """The oracle-only result of a case.  Computed once and shared; callers must not modify it."""
    return run(case, oracle_rows(CASES[case][0]).rows)
