"""sensing.channelModels.multiStaticChannel / multiStaticPaths (project-defined: include/isac_multistatic.h): the radar channel with paths from several
source arrays -- basicRadarChannel.m:39-64 with a transmit steering vector of its own per path -- and the host helper that turns geometry into the path list."""
from __future__ import annotations

import copy
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np

from ... import _lib as L
from ..radarParams import LIGHTSPEED, _db2pow, radarParams, steeringVector


def whole_sample_paths(paths, who):
    """ValueError for a record of multiStaticPaths(subSample=True) with a non-zero fraction, in a call whose model is the reference's whole-sample delay: the record's
    shift is floor(tau / Ts), one sample short of the ceil(tau / Ts) those calls document, and taking it silently would mis-round every path."""
    frac = getattr(paths, "frac", None)
    if frac is not None and np.any(np.asarray(frac, dtype=np.float64) != 0.0):
        raise ValueError(f"{who} delays by whole samples (ceil(tau / Ts)): a record with fractional delays (multiStaticPaths(subSample=True): shift = floor(tau / Ts)) is "
                         "served by multiStaticSensing in the spectral noise modes only")


class PathBlock:
    """The flat arrays of the two multi-static entry points, from (txWaveforms, radarParams, paths); keeps every host buffer alive for the call.  ``args``: ctx .. seed
    without the three noise arguments, in include/isac_multistatic.h's order.  A record with ``frac`` (multiStaticPaths(subSample=True)): ``frac`` [P] and ``args_frac``, the
    same with path_frac behind path_shift -- include/isac_subsample.h's order; ``frac`` is None for a record without it."""

    def __init__(self, ctx, txWaveforms, rp, paths):
        waves = list(txWaveforms)
        named = [w for w in waves if w is not None]
        if not named:
            raise ValueError("txWaveforms holds no waveform")
        self.dev = all(isinstance(w, L.DeviceArray) for w in named)
        if not self.dev and any(isinstance(w, L.DeviceArray) for w in named):
            raise ValueError("txWaveforms must be all DeviceArrays or all NumPy arrays")
        self.ctx = ctx or (named[0].ctx if self.dev else L.default_context())
        shapes = [None if w is None else tuple(w.shape if self.dev else np.shape(w)) for w in waves]
        self.T = int(next(s for s in shapes if s is not None)[0])
        if any(s is not None and (len(s) != 2 or s[0] != self.T) for s in shapes):
            raise ValueError("every source waveform must be [T x nAnts] with the same T")
        self.d_waves = [w if (w is None or self.dev) else self.ctx.to_device(L.as_c128_f(w)) for w in waves]
        self.A = int(rp.nTxAnts)
        src = np.ascontiguousarray(np.asarray(paths.source).reshape(-1), dtype=np.int32)
        P = src.size
        self.n_ants_src = np.ascontiguousarray([0 if s is None else s[1] for s in shapes], dtype=np.int32)
        self.ptrs = (C.c_void_p * len(waves))(*[None if d is None else d.ptr for d in self.d_waves])
        self.source = src
        self.shift = np.ascontiguousarray(np.asarray(paths.shift).reshape(-1), dtype=np.int64)
        self.doppler, self.gain = L.as_f64(paths.doppler), L.as_f64(paths.gain)
        tx = [np.asarray(b, dtype=np.complex128).reshape(-1) for b in paths.txSteering]
        self.rx = L.as_c128_f(np.asarray(paths.rxSteering, dtype=np.complex128).reshape(self.A, -1, order="F"))
        if not (self.shift.size == self.doppler.size == self.gain.size == len(tx) == self.rx.shape[1] == P):
            raise ValueError("paths: source, shift, doppler, gain, txSteering and rxSteering must describe the same number of paths")
        for p in range(P):
            if 0 <= src[p] < len(waves) and tx[p].size != self.n_ants_src[src[p]]:
                raise ValueError(f"paths.txSteering[{p}] must have one value per element of source {int(src[p])}")
        self.tx = np.ascontiguousarray(np.concatenate(tx)) if tx else np.zeros(0, dtype=np.complex128)
        p_ = lambda a: a.ctypes.data_as(C.c_void_p)
        self.args = (self.ctx.handle, self.ptrs, p_(self.n_ants_src), len(waves), self.T, float(rp.fc), float(rp.fs), float(rp.N0), self.A, P,
                     p_(self.source), p_(self.shift), p_(self.doppler), p_(self.gain), p_(self.tx), p_(self.rx))
        self.frac = L.as_f64(paths.frac) if getattr(paths, "frac", None) is not None else None
        if self.frac is not None:
            if self.frac.size != P:
                raise ValueError("paths.frac must have one value per path")
            self.args_frac = self.args[:12] + (p_(self.frac),) + self.args[12:]

    def noise(self, noise):
        """The noise argument on the device (kept alive with the block)."""
        self.d_noise = noise if (noise is None or isinstance(noise, L.DeviceArray)) else self.ctx.to_device(L.as_c128_f(noise))
        return self.d_noise


def multiStaticChannel(txWaveforms, radarParams, paths, *, noise=None, seed=None, ctx=None):
    """rxWaveform [T x nAnts] = the sum over ``paths`` of delayed, Doppler-shifted, scaled copies of the source waveforms, each summed over its source array with the path's
    transmit steering vector and spread over the receive array with its receive steering vector (isac_multi_static_channel_dev).

    ``txWaveforms``: one [T x nAnts_s] array per source -- DeviceArrays (the result stays in HBM) or NumPy arrays (NumPy result); None for a source no path names.
    ``radarParams``: fc, fs, N0 and nTxAnts (the receive array) of the receiving cell.  ``paths``: the record ``multiStaticPaths`` returns (source, shift, doppler [Hz], gain,
    txSteering, rxSteering).  ``noise`` / ``seed`` as in basicRadarChannel.  No path -> IsacError NO_LOS."""
    whole_sample_paths(paths, "multiStaticChannel")
    b = PathBlock(ctx, txWaveforms, radarParams, paths)
    mode = L.NOISE_INJECTED if noise is not None else (L.NOISE_PHILOX if seed is not None else L.NOISE_NONE)
    out = b.ctx.empty((b.T, b.A))
    b.ctx.check(b.ctx.lib.isac_multi_static_channel_dev(*b.args, mode, b.noise(noise), seed or 0, out))
    return out if b.dev else out.numpy()


def _direction(frm, to):
    """(azimuth, elevation) in degrees and range of `to` seen from `frm`: radarParams.m:12-14's cart2sph."""
    x, y, z = (float(v) for v in np.asarray(to, dtype=np.float64) - np.asarray(frm, dtype=np.float64))
    return np.rad2deg(np.arctan2(y, x)), np.rad2deg(np.arctan2(z, np.hypot(x, y))), np.sqrt(x * x + y * y + z * z)


def multiStaticPaths(rxCell, sources, targets, *, carrierInfo, waveInfo, directLoS=None, targetLoS=None, directLossdB=0.0, subSample=False):
    """The path list of one receiving cell from geometry (host helper; radarParams.py's own expressions: steeringVector with its lambda quirk, ceil(tau / Ts)).

    ``rxCell``: the receiving cell's parameters (what sensing.radarParams takes).  ``sources``: one cell-parameter record per transmitter, in the order of the waveform list
    (gNBPosition, gNBSenAntenna, gNBTxAnts, gNBRxGain); a source AT the receiver's position is the cell itself.  ``targets``: records with ``position`` [3], ``velocity`` [3]
    (a vector, m/s) and ``rcs``.  With v_n the target's speed towards node n, R_n its distance from it, At / Ar the source's / receiver's antenna gain:
      * target path j -> target -> i:  tau = (R_j + R_i) / c,  g = sqrt(At Ar lambda^2 sigma / ((4 pi)^3 R_j^2 R_i^2)),  f = (v_j + v_i) / lambda; each array steered at the target.
        For j = i the entry is EXACTLY radarParams' largeScaleFading, RxSteeringVec, ceil(2 R / c / Ts) and 2 v / lambda (it is taken from sensing.radarParams).
      * direct path j -> i (j != i):  tau = R_ji / c,  g = sqrt(At Ar lambda^2 / ((4 pi)^2 R_ji^2)) 10^(-directLossdB / 20),  f = 0; each array steered at the other.
    ``directLoS`` [S] and ``targetLoS`` [S x Q] are line-of-sight flags as isac_los_check_dev produces them (1 = LoS; None = all): a blocked path is left out.  The receiver's
    own row of ``targetLoS`` is that of the source at its position; where it is not among the sources, ``targetLoS`` has one more row, the receiver's, at the end.
    ``directLossdB``: a scalar or one value per source (a wall in an otherwise direct path).

    ``subSample`` (include/isac_subsample.h): True = no path is rounded up to a whole sample: shift = floor(tau / Ts) and the record gains ``frac`` = tau / Ts - shift in
    [0, 1), for every path, the receiver's own echoes included (tau = 2 R / c of sensing.radarParams' range); multiStaticSensing then takes the fractional-delay entry
    point.  False: the record of the reference's ceil, without ``frac``.

    Returns a namespace: source, shift, doppler, gain [P], txSteering (list of P vectors), rxSteering [nAnts x P], kind (per path: ("direct", j) or ("target", j, k))."""
    S, Q = len(sources), len(targets)
    pos_i = np.asarray(rxCell.gNBPosition, dtype=np.float64)
    fc = float(rxCell.dlCarrierFreq)
    lam = LIGHTSPEED / fc
    Ts = 1.0 / float(waveInfo.SampleRate)
    A, arr_i, Ar = int(rxCell.gNBTxAnts), rxCell.gNBSenAntenna, _db2pow(rxCell.gNBRxGain)
    own = [bool(np.array_equal(np.asarray(s.gNBPosition, dtype=np.float64), pos_i)) for s in sources]
    d_los = np.ones(S, dtype=bool) if directLoS is None else np.asarray(directLoS).reshape(S) == 1
    t_los = np.ones((S + 1, Q), dtype=bool) if targetLoS is None else np.asarray(targetLoS).reshape(-1, Q) == 1
    rx_row = own.index(True) if any(own) else S
    if t_los.shape[0] <= rx_row:
        raise ValueError("targetLoS needs the receiver's row: the receiver is not among the sources")
    loss = np.broadcast_to(np.asarray(directLossdB, dtype=np.float64), (S,))
    t_pos = [np.asarray(t.position, dtype=np.float64) for t in targets]
    t_vel = [np.asarray(t.velocity, dtype=np.float64) for t in targets]

    def speed_towards(k, node):
        d = t_pos[k] - node
        return float(-(t_vel[k] @ d) / np.sqrt(d @ d))

    mono = None
    if any(own) and Q:                                                      # the receiver's own echoes: sensing.radarParams itself on the same targets
        c = copy.copy(rxCell)
        c.numTargets, c.targetPosition = Q, np.stack(t_pos)
        c.rcs, c.velocity = np.array([float(t.rcs) for t in targets]), np.array([speed_towards(k, pos_i) for k in range(Q)])
        mono = radarParams(c, carrierInfo, waveInfo)
    out = SimpleNamespace(source=[], shift=[], doppler=[], gain=[], txSteering=[], rxSteering=[], kind=[])

    frac = []

    def add(j, delay, f, g, b, a, kind):                                    # delay: tau / Ts
        shift = np.floor(delay) if subSample else np.ceil(delay)
        frac.append(float(delay - shift) if subSample else 0.0)
        out.source.append(j); out.shift.append(int(shift)); out.doppler.append(float(f)); out.gain.append(float(g))
        out.txSteering.append(np.asarray(b, dtype=np.complex128)); out.rxSteering.append(np.asarray(a, dtype=np.complex128)); out.kind.append(kind)

    for j, s in enumerate(sources):
        pos_j, A_j, arr_j, At = np.asarray(s.gNBPosition, dtype=np.float64), int(s.gNBTxAnts), s.gNBSenAntenna, _db2pow(s.gNBRxGain)
        if not own[j] and d_los[j]:
            azi_ij, ele_ij, R = _direction(pos_i, pos_j)
            azi_ji, ele_ji, _ = _direction(pos_j, pos_i)
            g = math.sqrt(At * Ar * lam ** 2 / ((4.0 * np.pi) ** 2 * R ** 2)) * 10.0 ** (-float(loss[j]) / 20.0)
            add(j, R / LIGHTSPEED / Ts, 0.0, g, steeringVector(arr_j, A_j, lam, azi_ji, ele_ji), steeringVector(arr_i, A, lam, azi_ij, ele_ij), ("direct", j))
        for k in range(Q):
            if not (t_los[j, k] and t_los[rx_row, k]):
                continue
            if own[j]:
                add(j, 2.0 * mono.range[k] / LIGHTSPEED / Ts, 2.0 * mono.velocity[k] / lam, mono.largeScaleFading[k], mono.RxSteeringVec[:, k], mono.RxSteeringVec[:, k],
                    ("target", j, k))
                continue
            azi_j, ele_j, R_j = _direction(pos_j, t_pos[k])
            azi_i, ele_i, R_i = _direction(pos_i, t_pos[k])
            g = math.sqrt(At * Ar * lam ** 2 * float(targets[k].rcs) / ((4.0 * np.pi) ** 3 * (R_j * R_i) ** 2))   # (R_j R_i)^2: the same bits with j and i exchanged
            f = (speed_towards(k, pos_j) + speed_towards(k, pos_i)) / lam
            add(j, (R_j + R_i) / LIGHTSPEED / Ts, f, g, steeringVector(arr_j, A_j, lam, azi_j, ele_j), steeringVector(arr_i, A, lam, azi_i, ele_i), ("target", j, k))
    out.source, out.shift = np.asarray(out.source, dtype=np.int32), np.asarray(out.shift, dtype=np.int64)
    out.doppler, out.gain = np.asarray(out.doppler, dtype=np.float64), np.asarray(out.gain, dtype=np.float64)
    out.rxSteering = np.stack(out.rxSteering, axis=1) if out.rxSteering else np.zeros((A, 0), dtype=np.complex128)
    if subSample:
        out.frac = np.asarray(frac, dtype=np.float64)
    return out
