"""The C headers under include/ as the ABI tests read them: one parser of the `int isac_...(...)` declarations and one restatement of the binding's typing rule,
for include/isac.h and every additive header it includes.  The rule is restated here, not imported from the binding: by-value scalars by their C type, a pointer to
a struct of MIRRORS -> POINTER(mirror), every other pointer (T[] parameters included, and isac_target_list*, which is outside the mirror set) -> c_void_p."""
from __future__ import annotations

import ctypes
import os
import re

from conftest import ROOT

SCALARS = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t,
           "double": ctypes.c_double}
MIRRORS = {"isac_carrier": "Carrier", "isac_est_params": "EstParams", "isac_cfar_config": "CfarConfig", "isac_radar_channel_params": "RadarChannelParams",
           "isac_music2d_params": "Music2dParams", "isac_est_result": "EstResult", "isac_csi_report": "CsiReport", "isac_srs_report": "SrsReport",
           "isac_cdl_job": "CdlJob", "isac_sensing_job": "SensingJob", "isac_rx_frontend_job": "RxFrontendJob", "isac_path_loss_config": "PathLossConfig",
           "isac_cfar_method": "CfarMethod"}
RETURNS = {"int": ctypes.c_int, "const char*": ctypes.c_char_p}


def text(header):
    return open(os.path.join(ROOT, "include", header)).read()


def without_comments(header):
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text(header), flags=re.S))


def includes():
    """The additive headers, in the order of the #include "isac_*.h" lines of isac.h."""
    return re.findall(r'^#include "(isac_\w+\.h)"', text("isac.h"), flags=re.M)


def declarations(header):
    """[(return type, name, parameter text)] of every function the header declares, in its order."""
    return [(re.sub(r"\s*\*", "*", ret), name, " ".join(params.split()))
            for ret, name, params in re.findall(r"\b(int|const char\s*\*)\s+(isac_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", without_comments(header))]


def prototypes(header):
    """[(return type, name, [parameter type, ...])] of every function the header declares; `T name[n]` is the pointer `T*`."""
    out = []
    for ret, name, params in declarations(header):
        types = []
        for p in ([] if params == "void" else params.split(",")):
            m = re.fullmatch(r"(.*?)\s*\b\w+\s*(\[\d*\])?", p.strip())
            types.append(re.sub(r"\s*\*", "*", m.group(1)) + ("*" if m.group(2) else ""))
        out.append((ret, name, types))
    return out


def rule(c_type, L):
    if "*" not in c_type:
        return SCALARS[c_type]
    m = re.fullmatch(r"(?:const )?(isac_\w+)\*", c_type)
    return ctypes.POINTER(getattr(L, MIRRORS[m.group(1)])) if m and m.group(1) in MIRRORS else ctypes.c_void_p


def sizeof_selectors():
    """{selector: (header, NAME)} of every ISAC_SIZEOF_NAME, the enum form (`ISAC_SIZEOF_X = n`) and the macro form (`#define ISAC_SIZEOF_X n`), over all headers."""
    out = {}
    for header in ["isac.h"] + includes():
        for name, value in re.findall(r"\bISAC_SIZEOF_(\w+)(?: = |[ \t]+)(\d+)", without_comments(header)):
            assert int(value) not in out, (header, name, value)
            out[int(value)] = (header, name)
    return out
