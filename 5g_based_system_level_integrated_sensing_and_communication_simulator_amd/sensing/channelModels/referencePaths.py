"""sensing.channelModels.referencePaths (project-defined: include/isac_cancel_paths.h): the reference signals of sensing.cancelPaths from a path list."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from .multiStaticChannel import whole_sample_paths


def referencePaths(paths, kinds=("direct",), taps=0):
    """The references ``sensing.cancelPaths`` takes, from a ``multiStaticPaths`` record: the paths whose ``kind`` starts with one of ``kinds`` ("direct", "target"), in the
    record's order, each expanded to the shifts d - taps .. d + taps (ascending, clipped at 0); a reference that repeats an earlier one exactly -- same source, shift, Doppler
    and steering bits -- is left out, since a repeated column makes the fit singular.  Gains and receive steering vectors are not carried over: the fit finds them.

    A record with fractional delays (multiStaticPaths(subSample=True)) is refused with ValueError: the references are delayed by whole samples.

    Returns a namespace: source, shift, doppler [M], txSteering (list of M vectors), kind (per reference, the kind of the path it came from)."""
    whole_sample_paths(paths, "referencePaths")
    taps = int(taps)
    if taps < 0:
        raise ValueError("taps must be >= 0")
    out = SimpleNamespace(source=[], shift=[], doppler=[], txSteering=[], kind=[])
    seen = set()
    for p, kind in enumerate(paths.kind):
        if kind[0] not in kinds:
            continue
        b = np.ascontiguousarray(paths.txSteering[p], dtype=np.complex128).reshape(-1)
        s, d, f = int(paths.source[p]), int(paths.shift[p]), float(paths.doppler[p])
        for shift in range(max(d - taps, 0), d + taps + 1):
            key = (s, shift, np.float64(f).tobytes(), b.tobytes())
            if key in seen:
                continue
            seen.add(key)
            out.source.append(s); out.shift.append(shift); out.doppler.append(f); out.txSteering.append(b); out.kind.append(kind)
    out.source, out.shift = np.asarray(out.source, dtype=np.int32), np.asarray(out.shift, dtype=np.int64)
    out.doppler = np.asarray(out.doppler, dtype=np.float64)
    return out
