"""sensing.cancelPaths (project-defined: include/isac_cancel_paths.h): known reference signals projected out of a received waveform before OFDM
demodulation -- the answer to a neighbour's direct path in the waveform of sensing.channelModels.multiStaticChannel."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np

from .. import _lib as L
from .channelModels.multiStaticChannel import PathBlock, whole_sample_paths


def cancelPaths(rxWaveform, txWaveforms, radarParams, refs, *, loading=0.0, out=None, ctx=None, return_info=False):
    """rxWaveform [T x nAnts] less its least-squares fit by the reference signals ``refs`` (isac_cancel_paths_dev): every reference is a source waveform summed over its array
    with a transmit steering vector, delayed and Doppler-shifted like a path of multiStaticChannel, with unit gain; the fit finds one complex coefficient per reference and
    receive element.

    ``rxWaveform``: a DeviceArray (DeviceArray out; ``out`` may name the result's buffer, ``rxWaveform`` itself for in place) or a NumPy array (NumPy out).  ``txWaveforms``:
    one [T x nAnts_s] array per source as for multiStaticChannel, None for a source no reference names.  ``radarParams``: fc, fs and nTxAnts (the receive array).  ``refs``: the
    record ``sensing.channelModels.referencePaths`` returns (source, shift, doppler [Hz], txSteering).  ``loading`` >= 0: G_mm (1 + loading) on the Gram matrix's diagonal.
    A reference that is all zero or dependent on the ones before it: IsacError INVALID_ARG with ``.dependent`` = its index; nothing is written.

    ``return_info``: also a namespace with coef [nRefs x nAnts], power_in, power_out [nAnts] (sum |.|^2 before and after) and removed_dB = 10 log10(power_in / power_out)."""
    dev = isinstance(rxWaveform, L.DeviceArray)
    whole_sample_paths(refs, "cancelPaths")                                 # a multiStaticPaths(subSample=True) record handed over as it is
    src = np.ascontiguousarray(np.asarray(refs.source).reshape(-1), dtype=np.int32)
    M = int(src.size)
    A = int(radarParams.nTxAnts)
    unit = SimpleNamespace(source=src, shift=refs.shift, doppler=refs.doppler, gain=np.ones(M), txSteering=refs.txSteering, rxSteering=np.ones((A, M), dtype=np.complex128))
    rp = SimpleNamespace(fc=radarParams.fc, fs=radarParams.fs, N0=0.0, nTxAnts=A)
    b = PathBlock(ctx or (rxWaveform.ctx if dev else None), txWaveforms, rp, unit)
    shape = tuple(rxWaveform.shape if dev else np.shape(rxWaveform))
    if shape != (b.T, A):
        raise ValueError(f"rxWaveform must be [T x nTxAnts] = {(b.T, A)}")
    d_rx = rxWaveform if dev else b.ctx.to_device(L.as_c128_f(rxWaveform))
    if out is None or not dev:
        out = d_rx if not dev else b.ctx.empty(shape)                       # (a NumPy input's device copy is the call's own: in place)
    elif tuple(out.shape) != shape:
        raise ValueError(f"out must have shape {shape}")
    coef = np.zeros((M, A), dtype=np.complex128, order="F")
    power = np.zeros((2, A), dtype=np.float64)                                  # power_in [A], then power_out [A]
    dep = C.c_int32(-1)
    p_ = lambda a: a.ctypes.data_as(C.c_void_p)
    # ctx .. fs, n_ants, n_refs, source, shift, doppler, tx steering: the multi-static argument block without N0, the gains and the receive steering
    st = b.ctx.lib.isac_cancel_paths_dev(*b.args[:7], A, M, *b.args[10:13], b.args[14], float(loading), d_rx, out, p_(coef), p_(power), C.byref(dep))
    if st != 0:
        err = L.IsacError(st, (b.ctx.lib.isac_last_error(b.ctx.handle) or b"").decode())
        err.dependent = int(dep.value)
        raise err
    res = out if dev else out.numpy()
    if not return_info:
        return res
    with np.errstate(divide="ignore"):
        removed = 10.0 * np.log10(power[0] / power[1])
    return res, SimpleNamespace(coef=coef, power_in=power[0].copy(), power_out=power[1].copy(), removed_dB=removed)
