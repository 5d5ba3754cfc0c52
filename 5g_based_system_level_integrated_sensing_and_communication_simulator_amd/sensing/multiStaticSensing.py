"""sensing.multiStaticSensing (project-defined: include/isac_multistatic.h): monoStaticSensing.m:1-23 with an echo that holds paths from other cells'
transmitters."""
from __future__ import annotations

import ctypes as C

from .. import _lib as L
from ._marshal import carrier_block
from .channelModels.multiStaticChannel import PathBlock


def multiStaticSensing(txWaveforms, txDimension, carrierInfo, radarParams, paths, *, noise=None, seed=None, spectral_noise=None, noise_domain="time", nfft=None, ctx=None,
                       out=None):
    """echoGrid [nSc x nSym x nAnts] of a receiving cell that hears ``paths`` from several source arrays: sensing.channelModels.multiStaticChannel + OFDM demodulation +
    zero-padding of the symbol dimension up to ``txDimension(2)``, fused on the device (isac_multi_static_sensing_dev).  Hand the grid to ``fft2D`` with the transmit grid of
    whichever source is to be matched: the cell's own (sensing under interference) or a neighbour's (bistatic sensing).

    ``txWaveforms``: one [T x nAnts_s] array per source, DeviceArrays (DeviceArray out) or NumPy arrays (NumPy out); None for a source no path names.  ``radarParams``: fc, fs,
    N0 and nTxAnts (the receive array) of the receiving cell.  ``paths``: sensing.channelModels.multiStaticPaths' record.  ``noise`` / ``seed`` / ``spectral_noise`` /
    ``noise_domain`` / ``nfft`` / ``out``: as in monoStaticSensing; the noise field is that of the mono-static call with the same seed.  A record with ``frac``
    (multiStaticPaths(subSample=True)) goes to isac_multi_static_sensing_frac_dev (include/isac_subsample.h): non-zero fractions need a spectral noise mode
    (``spectral_noise`` or ``seed`` with ``noise_domain="spectral"``), else IsacError UNSUPPORTED."""
    b = PathBlock(ctx, txWaveforms, radarParams, paths)
    car = carrier_block(carrierInfo, nfft)
    if spectral_noise is not None:
        if noise is not None:
            raise ValueError("give either time-domain `noise` or `spectral_noise`, not both")
        mode, noise = L.NOISE_INJECTED_SPECTRAL, spectral_noise
    elif noise is not None:
        mode = L.NOISE_INJECTED
    elif seed is not None:
        if noise_domain not in ("time", "spectral"):
            raise ValueError("noise_domain must be 'time' or 'spectral'")
        mode = L.NOISE_PHILOX_SPECTRAL if noise_domain == "spectral" else L.NOISE_PHILOX
    else:
        mode = L.NOISE_NONE
    lib = b.ctx.lib
    lw = C.c_int32(0)
    st = lib.isac_ofdm_symbol_count(C.byref(car), b.T, C.byref(lw))
    if st != 0:
        raise L.IsacError(st, "isac_ofdm_symbol_count failed")
    shape = (car.n_sc, max(int(lw.value), int(txDimension[1]), 1), b.A)
    if out is None or not b.dev:
        out = b.ctx.empty(shape)
    elif tuple(out.shape) != shape:
        raise ValueError(f"out must have shape {shape}")
    lo = C.c_int32(0)
    tail = (mode, b.noise(noise), seed or 0, int(txDimension[1]), C.byref(car), out, C.byref(lo))
    if b.frac is not None:                                                  # a record of multiStaticPaths(subSample=True): include/isac_subsample.h
        b.ctx.check(lib.isac_multi_static_sensing_frac_dev(*b.args_frac, *tail))
    else:
        b.ctx.check(lib.isac_multi_static_sensing_dev(*b.args, *tail))
    return out if b.dev else out.numpy()
