"""NumPy restatement of reference-signal cancellation on the received waveform (include/isac_cancel_paths.h, DESIGN.md section 5 -- project-defined).  A reference column is
the single-path, unit-gain, single-element output of tests/_multistatic_restatement.multi_static_channel; the coefficients come from numpy.linalg.lstsq on the columns (an
orthogonal factorisation, not the normal equations the device solves), with `loading` from the loaded normal equations.  Also here: referencePaths restated, the random edge
cases tests/test_gpu_cancel.py runs, and the `interference` scene of _multistatic_restatement cancelled on the CPU.  Nothing here comes from the package under test."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import oracle as O
import _multistatic_restatement as M
import _numerology_scenes as N


def reference_columns(tx_waveforms, fc, fs, refs):
    """R [T x M]: refs is an iterable of (source, shift, doppler_hz, b [A_s])."""
    one = np.ones(1, dtype=np.complex128)
    return np.stack([M.multi_static_channel(tx_waveforms, fc, fs, 0.0, 1, [(s, d, f, 1.0, b, one)], None)[:, 0] for (s, d, f, b) in refs], axis=1)


def cancel(rx, tx_waveforms, fc, fs, refs, loading=0.0):
    """namespace(out [T x A], coef [M x A], power_in, power_out [A], R, G) of Y' = Y - R C."""
    Y = np.asarray(rx, dtype=np.complex128)
    R = reference_columns(tx_waveforms, fc, fs, refs)
    G = R.conj().T @ R
    if loading == 0.0:
        C = np.linalg.lstsq(R, Y, rcond=None)[0]
    else:
        Gl = G.copy()
        Gl[np.diag_indices_from(Gl)] *= 1.0 + loading
        C = np.linalg.solve(Gl, R.conj().T @ Y)
    out = Y - R @ C
    return SimpleNamespace(out=out, coef=C, power_in=(np.abs(Y) ** 2).sum(axis=0), power_out=(np.abs(out) ** 2).sum(axis=0), R=R, G=G)


def ref_tuples(r):
    """The tuples reference_columns takes, from a record with the fields of sensing.channelModels.referencePaths."""
    return [(int(r.source[i]), int(r.shift[i]), float(r.doppler[i]), np.asarray(r.txSteering[i])) for i in range(len(r.source))]


def reference_paths(rows, kinds=("direct",), taps=0):
    """referencePaths restated on the rows of _multistatic_restatement.restated_paths -- (source, shift, doppler, gain, b, a) -- and their kinds: every row of a listed kind at the
    shifts d - taps .. d + taps, clipped at 0; exact repeats dropped."""
    rows, kind = rows
    out = []
    for row, k in zip(rows, kind):
        if k[0] not in kinds:
            continue
        s, d, f, b = row[0], row[1], row[2], np.asarray(row[4], dtype=np.complex128)
        for shift in sorted({max(d + i, 0) for i in range(-taps, taps + 1)}):
            if not any(s == q[0] and shift == q[1] and np.float64(f).tobytes() == np.float64(q[2]).tobytes() and b.tobytes() == q[3].tobytes() for q in out):
                out.append((s, shift, f, b))
    return out


# ---------------------------------------------------------------- random edge cases: two sources of 2 and 3 elements
A_SRC = (2, 3)
FC = 3.5e9
FS = 30.72e6
# name -> (T, receive elements, references)
EDGE_CASES = {
    "t1000_a1_m1": (1000, 1, 1),          # the lone reference is the one-sample column (shift T - 1): G is 1 x 1
    "t1000_a3_m9": (1000, 3, 9),
    "t4099_a4_m16": (4099, 4, 16),        # one full reference tile
    "t4099_a3_m17": (4099, 3, 17),        # ... and one over: two row tiles
    "t1000_a4_m32": (1000, 4, 32),        # the limit, on the shortest waveform
    "t30720_a4_m32": (30720, 4, 32),      # ... and on the scene's length: more than one workgroup per pass
}
_edge = {}


def edge_case(name):
    """namespace(T, A, waves, refs (record), rows, Y, want (cancel's result), want_loaded (loading 0.1), cond): complex-normal source waveforms, unit-modulus steering phases,
    distinct shifts -- 0, T - 1 and T // 4 distinct values in between -- Doppler of both signs and zero, Y = R C0 + complex-normal noise of the references' size.  The column of
    shift T - 1 holds ONE sample: its steering vector is scaled so that the column has the energy of a full one (a steering vector is any complex vector), which keeps
    cond(G) <= 1e3 with that reference in the set.  Made once per process; arrays read-only."""
    if name in _edge:
        return _edge[name]
    T, A, n = EDGE_CASES[name]
    rng = np.random.default_rng(1000 * n + A)
    cn = lambda shape: np.asfortranarray(rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    waves = [cn((T, a)) for a in A_SRC]
    source = (np.arange(n) % 2).astype(np.int32)
    rng.shuffle(source)
    if n == 1:
        shift = np.array([T - 1], dtype=np.int64)
    else:
        mid = rng.choice(np.arange(1, T // 4), size=n - 2, replace=False) if n > 2 else np.zeros(0, dtype=np.int64)
        shift = np.concatenate([[0], mid, [T - 1]]).astype(np.int64)
    assert len(set(shift.tolist())) == n
    doppler = rng.uniform(-4e3, 4e3, n)
    doppler[::3] = 0.0
    if n > 1:
        doppler[1] = 2.5e3
    steer = [np.exp(2j * np.pi * rng.random(A_SRC[s])) for s in source]
    last = int(np.argmax(shift))
    beam0 = waves[source[last]][0, :] @ steer[last]                           # the one sample the column of shift T - 1 holds (times a unit phase)
    steer[last] = steer[last] * (np.sqrt(2.0 * T * A_SRC[source[last]]) / abs(beam0))
    refs = SimpleNamespace(source=source, shift=shift, doppler=doppler, txSteering=steer)
    rows = ref_tuples(refs)
    R = reference_columns(waves, FC, FS, rows)
    Y = np.asfortranarray(R @ (cn((n, A)) * 0.7) + cn((T, A)) * np.sqrt(2.5))
    v = SimpleNamespace(T=T, A=A, M=n, waves=waves, refs=refs, rows=rows, Y=Y, want=cancel(Y, waves, FC, FS, rows), want_loaded=cancel(Y, waves, FC, FS, rows, 0.1),
                        rp=SimpleNamespace(fc=FC, fs=FS, nTxAnts=A))
    v.cond = float(np.linalg.cond(v.want.G))
    for arr in waves + [Y, v.want.out, v.want.coef, v.want_loaded.out]:
        arr.setflags(write=False)
    _edge[name] = v
    return v


# ---------------------------------------------------------------- the `interference` scene of _multistatic_restatement, cancelled
DIRECT_SAMPLES = 43                                                          # the direct path's delay: 419 m
_scene = {}


def scene_kinds():
    """The kinds multiStaticPaths gives the rows of M.restated_paths("interference"): the own echo, the neighbour's direct path, its echo off the target."""
    return [("target", 0, 0), ("direct", 1), ("target", 1, 0)]


def interference(taps=0):
    """namespace(Y, refs, res, echo, est, dets, margin): the scene's waveform with its time-domain noise, the direct path's reference(s), the restated cancellation, the
    demodulated grid and oracle.fft2d on it with the cell's OWN transmit grid (est None where findpeaks raises), every antenna's CFAR list and guard margin."""
    if taps not in _scene:
        b = M.base()
        sc = b.sc
        rows = M.restated_paths("interference")
        waves = [sc.tx_wave, b.nb.tx_wave]
        Y = np.asfortranarray(M.multi_static_channel(waves, sc.rp.fc, sc.rp.fs, sc.rp.N0, sc.A, rows, sc.noise))
        refs = reference_paths((rows, scene_kinds()), ("direct",), taps)
        res = cancel(Y, waves, sc.rp.fc, sc.rp.fs, refs)
        case = N.CASE[M.SCENE_CASE]
        echo = np.asfortranarray(O.ofdm_demodulate(res.out, sc.K, sc.wave.Nfft, case.scs))
        assert echo.shape == (sc.K, sc.L, sc.A)
        cfg = O.cfar2d_config(sc.rp)
        rdm = O.rdm_explicit(echo, sc.tx_grid, int(sc.rp.nIFFT), int(sc.rp.nFFT))
        margin = tuple(N.guard_margin(np.abs(rdm[:, :, a]) ** 2, cfg.CUTIdx, cfg.Pfa) for a in range(sc.A))
        dets = [O.ca_cfar2d(np.abs(rdm[:, :, a]) ** 2, cfg.CUTIdx, cfg.Pfa, cfg.GuardBandSize, cfg.TrainingBandSize) for a in range(sc.A)]
        try:
            est = O.fft2d(sc.rp, cfg, echo, sc.tx_grid, rdm_fn=O.rdm_explicit)
        except ValueError:
            est = None
        for arr in (Y, res.out, echo):
            arr.setflags(write=False)
        _scene[taps] = SimpleNamespace(Y=Y, waves=waves, refs=refs, res=res, echo=echo, est=est, dets=dets, margin=margin, cfg=cfg)
    return _scene[taps]
