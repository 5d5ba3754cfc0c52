"""applyChannelModel of the two PHYs (uePhy.m:724-755 downlink, gNBPhy.m:833-864 uplink), whole: the channel object (or the DFT matrix of a link without one),
then path loss, receiver gain and thermal noise on the device, in place on the channel's output (isac_rx_frontend[_batch]_dev)."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ... import _lib as L
from ..channelModels.cdl import applyCDL, applyCDLBatch
from ..pathlossModels import config5GNRModels, configFreeSpaceModel


def thermalNoisePower(temperature_k, noise_figure_db, sample_rate):
    """Nt [W] = k (T + 290 (10^(F/10) - 1)) fs   (uePhy.m:942-950, gNBPhy.m:1071-1080) -- isac_thermal_noise_power."""
    out = C.c_double(0.0)
    st = L.load().isac_thermal_noise_power(float(temperature_k), float(noise_figure_db), float(sample_rate), C.byref(out))
    if st != 0:
        raise L.IsacError(st, "isac_thermal_noise_power")
    return out.value


def dftChannelMatrix(n_tx, n_rx):
    """H [n_tx x n_rx] = fft(eye(n)); H = H(1:n_tx, 1:n_rx); H = H / norm(H), n = max(n_tx, n_rx)   (uePhy.m:732-740) -- isac_dft_channel_matrix."""
    h = np.zeros((int(n_tx), int(n_rx)), dtype=np.complex128, order="F")
    st = L.load().isac_dft_channel_matrix(int(n_tx), int(n_rx), h.ctypes.data_as(C.c_void_p))
    if st != 0:
        raise L.IsacError(st, "isac_dft_channel_matrix: antenna counts must be positive")
    return h


def pathLoss(path_loss_config, carrier_freq, los, own_position, tx_position):
    """The branch of uePhy.m:742-747 / gNBPhy.m:851-856: 'fspl' -> configFreeSpaceModel, anything else -> config5GNRModels.  Positions in the reference's argument order
    (the receiver's own node first, the packet's transmitter second) -- see config5GNRModels for what that does to the heights in the downlink."""
    if path_loss_config == "fspl":
        return configFreeSpaceModel(carrier_freq, own_position, tx_position)
    return config5GNRModels(path_loss_config, carrier_freq, los, own_position, tx_position)


def rxFrontEndBatch(arrays, path_scales, gain_scales, noise_powers, *, seeds=None, noises=None, ctx=None):
    """In place on the DeviceArrays ``arrays`` (one shape [T x Nr]), one launch: y = (y * path_scale) * gain_scale + sqrt(Nt / 2) w.  ``noises`` (DeviceArrays of unit
    randn + 1j randn): injected mode; ``seeds``: Philox; neither: noiseless.  Asynchronous on the context's stream.  Returns ``arrays``."""
    arrays = list(arrays)
    if not arrays:
        return arrays
    if seeds is not None and noises is not None:
        raise ValueError("give `noises` (injected) or `seeds` (Philox), not both")
    ctx = ctx or arrays[0].ctx
    T, nr = arrays[0].shape
    n = len(arrays)
    mode = L.NOISE_INJECTED if noises is not None else (L.NOISE_PHILOX if seeds is not None else L.NOISE_NONE)
    jobs = (L.RxFrontendJob * n)()
    for j, a in enumerate(arrays):
        if not isinstance(a, L.DeviceArray) or tuple(a.shape) != (T, nr) or a.dtype != np.complex128:
            raise ValueError("rxFrontEndBatch: complex DeviceArrays of one shape [T x Nr]")
        w = None
        if noises is not None:
            w = noises[j]
            if not isinstance(w, L.DeviceArray) or tuple(w.shape) != (T, nr):
                raise ValueError("rxFrontEndBatch: `noises` must be DeviceArrays [T x Nr]")
        jobs[j] = L.RxFrontendJob(a.ptr, w.ptr if w is not None else None, float(path_scales[j]), float(gain_scales[j]), float(noise_powers[j]),
                                  int(seeds[j]) & 0xFFFFFFFFFFFFFFFF if seeds is not None else 0)
    ctx.check(ctx.lib.isac_rx_frontend_batch_dev(ctx.handle, jobs, n, T, nr, mode))
    if noises is not None:
        for a, w in zip(arrays, noises):
            a._rxfe_keep = w                        # the launch is asynchronous: the noise stays alive as long as the output does
    return arrays


def _scales(path_loss_config, carrier_freq, los, own_position, tx_position, rx_gain_db, noise_figure_db, temperature_k, sample_rate):
    pl = pathLoss(path_loss_config, carrier_freq, los, own_position, tx_position)
    return 10.0 ** (-pl / 20.0), 10.0 ** (float(rx_gain_db) / 20.0), thermalNoisePower(temperature_k, noise_figure_db, sample_rate)


def _dft_apply(d_x, n_rx, ctx):
    """waveform * H (the `else` branch) through isac_cdl_apply_dev: one path, one unit tap, shift 0, one gain block."""
    T, nt = d_x.shape
    h = dftChannelMatrix(nt, n_rx)
    hb = np.ascontiguousarray(h)                                          # [s][u], u fastest: the apply's layout of one path's gains
    start = np.zeros(1, dtype=np.int64)
    tap = np.ones(1, dtype=np.float64)
    shift = np.zeros(1, dtype=np.int32)
    d_y = ctx.empty((T, int(n_rx)))
    ctx.check(ctx.lib.isac_cdl_apply_dev(ctx.handle, d_x, T, nt, int(n_rx), 1, hb.ctypes.data_as(C.c_void_p), 1, start.ctypes.data_as(C.c_void_p),
                                         tap.ctypes.data_as(C.c_void_p), 1, shift.ctypes.data_as(C.c_void_p), 1.0, d_y))
    return d_y


def applyChannelModel(waveform, *, channel, n_rx=None, path_loss_config, carrier_freq, los, own_position, tx_position, rx_gain_db, noise_figure_db,
                      temperature_k, sample_rate, seed=None, noise=None, ctx=None):
    """rxWaveform = applyChannelModel(obj, pktInfo) for one link.  waveform [T x Nt] (numpy in -> numpy out, DeviceArray in -> DeviceArray out).
    ``channel``: a CDLChannel -> applyCDL exactly as a direct call (its time advances); None -> the DFT-matrix branch into ``n_rx`` receive elements.
    Then, on the device and in place: db2mag(-pathLoss), 10^(RxGain/20), + sqrt(Nt/2) w.  ``noise`` ([T x Nr] randn + 1j randn, array or DeviceArray): injected
    (parity) mode; ``seed``: the library's Philox stream; neither: noiseless.
    Not mirrored: the MaxChannelDelay zero rows uePhy.m:729 appends in front of the channel call -- the caller pads, as with applyCDL."""
    dev = isinstance(waveform, L.DeviceArray)
    ctx = ctx or (waveform.ctx if dev else L.default_context())
    d_x = waveform if dev else ctx.to_device(L.as_c128_f(waveform))
    if channel is not None:
        d_y = applyCDL(channel, d_x, ctx=ctx)
    else:
        if n_rx is None:
            raise ValueError("applyChannelModel: channel=None needs n_rx")
        d_y = _dft_apply(d_x, n_rx, ctx)
    s1, s2, nt_w = _scales(path_loss_config, carrier_freq, los, own_position, tx_position, rx_gain_db, noise_figure_db, temperature_k, sample_rate)
    d_w = None
    if noise is not None:
        d_w = noise if isinstance(noise, L.DeviceArray) else ctx.to_device(L.as_c128_f(noise))
    rxFrontEndBatch([d_y], [s1], [s2], [nt_w], seeds=None if seed is None or d_w is not None else [seed], noises=None if d_w is None else [d_w], ctx=ctx)
    return d_y if dev else d_y.numpy()


def applyChannelModelBatch(waveforms, *, channels, path_loss_config, carrier_freq, los, own_positions, tx_positions, rx_gain_db, noise_figure_db,
                           temperature_k, sample_rate, seeds=None, noises=None, ctx=None, outs=None, gains=None):
    """The UEs of a cell-slot: applyCDLBatch (one call) then the front end on its outputs (one launch).  ``waveforms``: DeviceArrays [T x Nt] (one per job; the same
    array may appear several times); ``channels``: one CDLChannel per job; ``los`` / ``own_positions`` / ``tx_positions``: one entry per job (the receiver's own node
    first, as in the reference's calls); the receiver parameters are shared.  ``noises`` / ``seeds``: one per job.  Returns the output DeviceArrays [T x Nr]."""
    channels, waveforms = list(channels), list(waveforms)
    ctx = ctx or waveforms[0].ctx
    ys = applyCDLBatch(channels, waveforms, ctx=ctx, outs=outs, gains=gains)
    n = len(ys)
    los = list(los) if np.ndim(los) else [los] * n
    sc = [_scales(path_loss_config, carrier_freq, los[j], own_positions[j], tx_positions[j], rx_gain_db, noise_figure_db, temperature_k, sample_rate) for j in range(n)]
    return rxFrontEndBatch(ys, [s[0] for s in sc], [s[1] for s in sc], [s[2] for s in sc], seeds=seeds, noises=noises, ctx=ctx)
