"""sensing.estimation.beamDetect: CFAR on beam planes of the last fft2D call (project-defined; include/isac_beams.h, isac_fft2d_beam_detect)."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np

from ... import _lib as L
from ..detection.cfarDetect import method_block


def beamDetect(ctx, W, Method="CA", Rank=1, ThresholdFactor="Auto", CustomThresholdFactor=None, beamAzimuth=None, return_debug=False):
    """The per-target list of the last completed fft2D on ``ctx`` with the array combined coherently BEFORE the detector: the complex range-Doppler window is weighted by
    every column of ``W`` [A x B] (sensing.estimation.beamWeights gives matched columns), each beam plane |w' y|^2 / (w' w) goes through detector ``Method`` ('CA', 'GOCA',
    'SOCA', 'OS'; ``Rank`` for 'OS') with ``ThresholdFactor`` 'Auto' or 'Custom' on the CUT zone fft2D was given, and the cells any beam detects are thinned to the local
    maxima of the map "strongest beam per cell".  Returns the dict of sensing.estimation.targetList (``power`` = that maximum, ``hits`` = beams that detect the cell) plus
    ``beam`` (1-based column of W with the maximum); ``azi`` = ``beamAzimuth[beam - 1]``, or the beam number when ``beamAzimuth`` is None.  ``return_debug`` adds a
    namespace with the per-beam ``detections`` ([2 x D] 1-based, CUT order), ``det_pow`` and ``beam_pow`` [nr x nc x B].
    Raises IsacError(INVALID_ARG) when no completed fft2D is left on the context."""
    lib = ctx.lib
    m = method_block(Method, Rank, ThresholdFactor, CustomThresholdFactor)
    dims = (C.c_int32 * 3)()
    ctx.check(lib.isac_fft2d_get_power_window(ctx.handle, None, 0, dims, None, None))
    w = L.as_c128_f(W)
    if w.ndim != 2 or w.shape[0] != int(dims[2]):
        raise ValueError(f"W must be [A x B] with A = {int(dims[2])}")
    B = w.shape[1]
    azi = None
    if beamAzimuth is not None:
        azi = L.as_f64(beamAzimuth)
        if azi.size != B:
            raise ValueError("beamAzimuth needs one label per column of W")
    out = L.TargetList()
    beam = np.zeros(L.ISAC_MAX_TARGETS, dtype=np.int32)
    off = np.zeros(B + 1, dtype=np.int32)
    n_total = C.c_int32(0)
    cap, idx, pw, bp = 1 << 30, None, None, None
    if return_debug:                                     # every list fits: a beam detects each cell of the window at most once
        cap = min(int(dims[0]) * int(dims[1]) * B, (1 << 31) - 1)
        idx = np.zeros((2, cap), dtype=np.int32, order="F")
        pw = np.zeros(cap, dtype=np.float64)
        bp = np.zeros((int(dims[0]), int(dims[1]), B), dtype=np.float64, order="F")
    st = lib.isac_fft2d_beam_detect(ctx.handle, w.ctypes.data_as(C.c_void_p), B, None if azi is None else azi.ctypes.data_as(C.c_void_p), C.byref(m), C.byref(out),
                                    beam.ctypes.data_as(C.c_void_p), None if idx is None else idx.ctypes.data_as(C.c_void_p),
                                    None if pw is None else pw.ctypes.data_as(C.c_void_p), cap, off.ctypes.data_as(C.c_void_p), C.byref(n_total),
                                    None if bp is None else bp.ctypes.data_as(C.c_void_p))
    ctx.check(st)
    n = int(out.n_targets)
    res = {"rng": np.array(out.rng[:n]), "vel": np.array(out.vel[:n]), "azi": np.array(out.azi[:n]), "power": np.array(out.power[:n]),
           "hits": np.array(out.hits[:n], dtype=np.int32), "row": np.array(out.row[:n], dtype=np.int32), "col": np.array(out.col[:n], dtype=np.int32),
           "beam": beam[:n].copy(), "n_total": int(out.n_total)}
    if not return_debug:
        return res
    dbg = SimpleNamespace(detections=[idx[:, off[b]:off[b + 1]].astype(np.int64) for b in range(B)], det_pow=[pw[off[b]:off[b + 1]] for b in range(B)], beam_pow=bp,
                          totalDetections=int(n_total.value))
    return res, dbg
