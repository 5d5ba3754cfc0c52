"""NumPy restatement of the multi-static radar channel (include/isac_multistatic.h, DESIGN.md section 5 -- project-defined): basicRadarChannel.m:39-64 with a path list
instead of a target list, written in basicRadarChannel's own order of operations (oracle/radar_channel.py line by line, `sv[:, i]` of :51 split into the path's transmit and
receive steering vectors, the source waveform chosen per path).  With mono-static paths it is oracle.basic_radar_channel bit for bit (tests/test_multistatic_cpu.py).
Also here: the path parameters of a geometry restated from the formulas of DESIGN.md section 5, and the three physical scenes both test files run.  Nothing here comes from the package
under test."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import oracle as O
import _numerology_scenes as N


def multi_static_channel(tx_waveforms, fc, fs, n0, n_ants, paths, noise_unit):
    """tx_waveforms: list of [T x A_s] (None where no path names the source); paths: iterable of (source, shift, doppler_hz, gain, b [A_s], a [n_ants]); noise_unit [T x n_ants]
    with N(0, 1) parts or None.  Returns rxWaveform [T x n_ants]; no path: ValueError (the empty rxWaveform of :59,64)."""
    t_len = next(np.asarray(x).shape[0] for x in tx_waveforms if x is not None)      # :8
    ts = 1.0 / fs                                                                   # :15
    t_axis = np.arange(t_len, dtype=np.float64) * ts                                # :29
    phase_tx = np.exp(2j * np.pi * fc * t_axis)                                     # :30
    up = {}
    echoes = []
    for (s, shift, fd, gain, b, a) in paths:
        if s not in up:
            up[s] = np.asarray(tx_waveforms[s], dtype=np.complex128) * phase_tx[:, None]   # :31
        tx = up[s]
        sft = min(int(shift), t_len)                                                # a path at or beyond T contributes nothing
        e = np.concatenate([np.zeros((sft, tx.shape[1]), dtype=np.complex128), tx[: t_len - sft]], axis=0)   # :42
        ph = np.exp(2j * np.pi * fd * (np.arange(e.shape[0], dtype=np.float64) * ts))                        # :43-44
        e = e * ph[:, None]                                                         # :45
        e = e * gain                                                                # :48
        e = (e @ np.asarray(b, dtype=np.complex128))[:, None] * np.asarray(a, dtype=np.complex128)[None, :]  # :51  (e*b)*a.'
        echoes.append(e)
    if not echoes:
        raise ValueError("no path -> empty rxWaveform")
    rx = echoes[0]
    for e in echoes[1:]:                                                            # :64
        rx = rx + e
    if noise_unit is not None:                                                      # :67-69
        rx = rx + np.sqrt(n0 / 2.0) * noise_unit
    phase_rx = np.exp(-2j * np.pi * fc * (np.arange(rx.shape[0], dtype=np.float64) * ts))   # :72-73
    return rx * phase_rx[:, None]                                                   # :74


def multi_static_sensing(tx_waveforms, tx_dim_l, n_sc, nfft, scs, fc, fs, n0, n_ants, paths, noise_unit):
    """monoStaticSensing.m:13-21 on the channel above -> echoGrid [n_sc x max(L, tx_dim_l) x n_ants]."""
    grid = O.ofdm_demodulate(multi_static_channel(tx_waveforms, fc, fs, n0, n_ants, paths, noise_unit), n_sc, nfft, scs)
    if grid.shape[1] < tx_dim_l:
        grid = np.concatenate([grid, np.zeros((grid.shape[0], tx_dim_l - grid.shape[1], grid.shape[2]), dtype=np.complex128)], axis=1)
    return grid


def path_tuples(p):
    """The tuples multi_static_channel takes, from a record with the fields of sensing.channelModels.multiStaticPaths."""
    return [(int(p.source[i]), int(p.shift[i]), float(p.doppler[i]), float(p.gain[i]), np.asarray(p.txSteering[i]), np.asarray(p.rxSteering)[:, i]) for i in range(len(p.source))]


def mono_static_paths(rp, los):
    """The LoS targets of a radarParams record as paths of source 0: d = ceil(2 R / c / Ts) (:21-22), f = 2 v / lambda (:25), g = largeScaleFading, b = a = RxSteeringVec."""
    lam, ts = O.LIGHTSPEED / rp.fc, 1.0 / rp.fs
    shift = np.ceil(2.0 * np.asarray(rp.range, dtype=np.float64) / O.LIGHTSPEED / ts).astype(np.int64)
    fd = 2.0 * np.asarray(rp.velocity, dtype=np.float64) / lam
    sv = np.asarray(rp.RxSteeringVec)
    keep = [i for i in range(int(rp.nTargets)) if np.asarray(los).reshape(-1)[i] == 1]
    return SimpleNamespace(source=np.zeros(len(keep), dtype=np.int32), shift=shift[keep], doppler=fd[keep], gain=np.asarray(rp.largeScaleFading, dtype=np.float64)[keep],
                           txSteering=[sv[:, i] for i in keep], rxSteering=sv[:, keep])


# ---------------------------------------------------------------- geometry, restated from the formulas of DESIGN.md section 5 (ULA nodes)
def _sph(frm, to):
    x, y, z = np.asarray(to, dtype=np.float64) - np.asarray(frm, dtype=np.float64)
    return np.rad2deg(np.arctan2(y, x)), np.sqrt(x * x + y * y + z * z)


def _ula(cell, lam, azi):
    return np.exp(2j * np.pi * (np.arange(int(cell.gNBTxAnts)) * cell.gNBSenAntenna.d) * O.sind(azi) / lam)       # radarParams.m:102-114, the lambda quirk included


def bistatic_path(src, rx, lam, ts, pos, vel, rcs):
    """(shift, f, g, b, a) of src -> target -> rx."""
    azi_j, r_j = _sph(src.gNBPosition, pos)
    azi_i, r_i = _sph(rx.gNBPosition, pos)
    at, ar = float(O.db2pow(src.gNBRxGain)), float(O.db2pow(rx.gNBRxGain))
    v = lambda node: -float(np.dot(vel, np.asarray(pos, dtype=np.float64) - np.asarray(node, dtype=np.float64))) / _sph(node, pos)[1]
    g = np.sqrt(at * ar * lam ** 2 * rcs / ((4.0 * np.pi) ** 3 * r_j ** 2 * r_i ** 2))
    return int(np.ceil((r_j + r_i) / O.LIGHTSPEED / ts)), (v(src.gNBPosition) + v(rx.gNBPosition)) / lam, g, _ula(src, lam, azi_j), _ula(rx, lam, azi_i)


def direct_path(src, rx, lam, ts, loss_db):
    """(shift, f, g, b, a) of src -> rx."""
    azi_ij, r = _sph(rx.gNBPosition, src.gNBPosition)
    azi_ji, _ = _sph(src.gNBPosition, rx.gNBPosition)
    at, ar = float(O.db2pow(src.gNBRxGain)), float(O.db2pow(rx.gNBRxGain))
    g = np.sqrt(at * ar * lam ** 2 / ((4.0 * np.pi) ** 2 * r ** 2)) * 10.0 ** (-loss_db / 20.0)
    return int(np.ceil(r / O.LIGHTSPEED / ts)), 0.0, g, _ula(src, lam, azi_ji), _ula(rx, lam, azi_ij)


# ---------------------------------------------------------------- the three physical scenes: scs60_nrb24_a4, its own target at (150, 40, 1.5), a second gNB at
# (400, 120, 30) with a waveform of its own
SCENE_CASE = "scs60_nrb24_a4"
NEIGHBOUR = (400.0, 120.0, 30.0)
SCENES = {
    "bistatic": dict(direct_los=0, loss_db=0.0),          # the neighbour's LoS to the receiver blocked: its echo off the target only
    "interference": dict(direct_los=1, loss_db=0.0),      # ... with its free-space direct path
    "wall": dict(direct_los=1, loss_db=40.0),             # ... with that path 40 dB down
}

_base = {}


def base():
    """namespace(sc, nb, targets): the table scene (own cell, source 0), the neighbour's cell record and waveform / grid (source 1, seed of its own), the target list with
    velocity vectors.  Made once per process; arrays read-only."""
    if not _base:
        sc = N.scene_of(N.CASE[SCENE_CASE])
        other = N.scene_of(N.CASE[SCENE_CASE], seed=2, with_noise=False)
        cell = O.default_cell_params(n_ants=sc.A, target_pos=N.CASE[SCENE_CASE].targets, velocity=N.CASE[SCENE_CASE].velocity)
        cell.numSlots = sc.cell.numSlots
        cell.gNBPosition = np.array(NEIGHBOUR)
        targets = [SimpleNamespace(position=np.asarray(p, dtype=np.float64), velocity=np.zeros(3), rcs=1.0) for p in N.CASE[SCENE_CASE].targets]
        for arr in (sc.tx_wave, sc.tx_grid, sc.noise, other.tx_wave, other.tx_grid):
            arr.setflags(write=False)
        _base["v"] = SimpleNamespace(sc=sc, nb=SimpleNamespace(cell=cell, tx_wave=other.tx_wave, tx_grid=other.tx_grid), targets=targets)
    return _base["v"]


def restated_paths(name):
    """The scene's path list from the formulas above: the own echo (radarParams' fields), the neighbour's direct path where it is in line of sight, its echo off the target."""
    b, kw = base(), SCENES[name]
    sc = b.sc
    lam, ts = O.LIGHTSPEED / sc.rp.fc, 1.0 / sc.rp.fs
    own = mono_static_paths(sc.rp, sc.los)
    rows = [(0, int(own.shift[i]), float(own.doppler[i]), float(own.gain[i]), own.txSteering[i], own.rxSteering[:, i]) for i in range(len(own.source))]
    if kw["direct_los"]:
        rows.append((1,) + direct_path(b.nb.cell, sc.cell, lam, ts, kw["loss_db"]))
    for t in b.targets:
        rows.append((1,) + bistatic_path(b.nb.cell, sc.cell, lam, ts, t.position, t.velocity, t.rcs))
    return rows


_scene = {}


def scene(name):
    """namespace(paths, echo, own, nbr, margin_own, margin_nbr): the restated paths, the restatement's echo grid with the scene's time-domain noise, and oracle.fft2d on it with
    the cell's own transmit grid and with the neighbour's -- (est | None, debug) each, None where findpeaks raises on an empty detection list -- and the guard margins."""
    if name not in _scene:
        b = base()
        sc = b.sc
        rows = restated_paths(name)
        case = N.CASE[SCENE_CASE]
        echo = np.asfortranarray(multi_static_sensing([sc.tx_wave, b.nb.tx_wave], sc.L, sc.K, sc.wave.Nfft, case.scs, sc.rp.fc, sc.rp.fs, sc.rp.N0, sc.A, rows, sc.noise))
        echo.setflags(write=False)
        cfg = O.cfar2d_config(sc.rp)

        def run(tx_grid):
            rdm = O.rdm_explicit(echo, tx_grid, int(sc.rp.nIFFT), int(sc.rp.nFFT))
            margin = tuple(N.guard_margin(np.abs(rdm[:, :, a]) ** 2, cfg.CUTIdx, cfg.Pfa) for a in range(sc.A))
            dets = [O.ca_cfar2d(np.abs(rdm[:, :, a]) ** 2, cfg.CUTIdx, cfg.Pfa, cfg.GuardBandSize, cfg.TrainingBandSize) for a in range(sc.A)]
            try:
                est = O.fft2d(sc.rp, cfg, echo, tx_grid, rdm_fn=O.rdm_explicit)
            except ValueError:
                est = None
            return est, dets, margin
        _scene[name] = SimpleNamespace(paths=rows, echo=echo, cfg=cfg, own=run(sc.tx_grid), nbr=run(b.nb.tx_grid))
    return _scene[name]
