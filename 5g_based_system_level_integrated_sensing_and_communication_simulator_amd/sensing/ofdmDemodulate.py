"""sensing.ofdmDemodulate: monoStaticSensing.m:16-21 on a waveform that already exists -- nrOFDMDemodulate and the zero-padding of the symbol dimension
(isac_ofdm_demodulate_dev).  With it the chain multiStaticChannel -> cancelPaths -> ofdmDemodulate -> fft2D stays in the package."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib as L
from ._marshal import carrier_block


def ofdmDemodulate(rxWaveform, txDimension, carrierInfo, nfft=None, ctx=None):
    """echoGrid [nSc x max(symbols, txDimension(2)) x nAnts] of rxWaveform [T x nAnts]: the whole OFDM symbols of the waveform, demodulated, and zero columns up to the
    transmit grid's symbol count.  A DeviceArray gives a DeviceArray, a NumPy array a NumPy array.  ``nfft``: as in monoStaticSensing."""
    dev = isinstance(rxWaveform, L.DeviceArray)
    ctx = ctx or (rxWaveform.ctx if dev else L.default_context())
    d_wave = rxWaveform if dev else ctx.to_device(L.as_c128_f(rxWaveform))
    if len(d_wave.shape) != 2:
        raise ValueError("rxWaveform must be [T x nAnts]")
    T, A = d_wave.shape
    car = carrier_block(carrierInfo, nfft)
    lw = C.c_int32(0)
    st = ctx.lib.isac_ofdm_symbol_count(C.byref(car), T, C.byref(lw))
    if st != 0:
        raise L.IsacError(st, "isac_ofdm_symbol_count failed")
    n_sym = max(int(lw.value), int(txDimension[1]), 1)
    out = ctx.empty((car.n_sc, n_sym, A))
    ctx.check(ctx.lib.isac_ofdm_demodulate_dev(ctx.handle, d_wave, T, A, C.byref(car), out, n_sym))
    return out if dev else out.numpy()
