"""NumPy / math restatement of the tail of applyChannelModel (uePhy.m:724-755, gNBPhy.m:833-864), written from TR 38.901 V16 Table 7.4.1-1 as the project's issue
transcribes it and from the reference lines cited below -- independent of csrc/rxfe.hip (nothing shared beyond Boltzmann's constant and c).  TEST INFRASTRUCTURE ONLY.

Scalars are evaluated with Python's ``math`` (the C library's log10 / pow, one value at a time): the library's host functions call the same routines, so the two sides
differ by the rounding of a few additions only (bound in tests/test_rx_frontend_cpu.py)."""
from __future__ import annotations

import math

import numpy as np

C0 = 299792458.0            # physconst('LightSpeed')
KB = 1.380649e-23           # physconst('Boltzmann')
SCENARIOS = ("UMa", "UMi", "RMa", "InH", "InF-SL", "InF-DL", "InF-SH", "InF-DH", "InF-HH")
L10 = math.log10


def geometry(bs, ue):
    """(d2D, d3D, hBS, hUT): the third coordinate of the FIRST position is hBS, of the second hUT."""
    d2 = math.sqrt((ue[0] - bs[0]) ** 2 + (ue[1] - bs[1]) ** 2)
    return d2, math.sqrt(d2 * d2 + (bs[2] - ue[2]) ** 2), float(bs[2]), float(ue[2])


def breakpoint_uma_umi(fc, hb, hu, he=1.0):
    return 4.0 * (hb - he) * (hu - he) * fc / C0


def breakpoint_rma(fc, hb, hu):
    return 2.0 * math.pi * hb * hu * fc / C0


def uma_los_branches(d, f, dbp, hb, hu):
    return 28.0 + 22.0 * L10(d) + 20.0 * L10(f), 28.0 + 40.0 * L10(d) + 20.0 * L10(f) - 9.0 * L10(dbp ** 2 + (hb - hu) ** 2)


def umi_los_branches(d, f, dbp, hb, hu):
    return 32.4 + 21.0 * L10(d) + 20.0 * L10(f), 32.4 + 40.0 * L10(d) + 20.0 * L10(f) - 9.5 * L10(dbp ** 2 + (hb - hu) ** 2)


def rma_pl1(d, f, h):
    return 20.0 * L10(40.0 * math.pi * d * f / 3.0) + min(0.03 * h ** 1.72, 10.0) * L10(d) - min(0.044 * h ** 1.72, 14.77) + 0.002 * L10(h) * d


def rma_los_branches(d, f, dbp, h):
    return rma_pl1(d, f, h), rma_pl1(dbp, f, h) + 40.0 * L10(d / dbp)


def path_loss_38901(scenario, fc, los, bs, ue, h=5.0, w=20.0, he=1.0):
    """nrPathLoss(nrPathLossConfig('Scenario', scenario), fc, los, bs, ue), defaults of nrPathLossConfig, OptionalModel off; 0 for equal positions."""
    if tuple(bs) == tuple(ue):
        return 0.0
    d2, d, hb, hu = geometry(bs, ue)
    f = fc / 1e9
    if scenario in ("UMa", "UMi"):
        dbp = breakpoint_uma_umi(fc, hb, hu, he)
        pl1, pl2 = (uma_los_branches if scenario == "UMa" else umi_los_branches)(d, f, dbp, hb, hu)
        pl_los = pl1 if d2 <= dbp else pl2
        if scenario == "UMa":
            pl_n = 13.54 + 39.08 * L10(d) + 20.0 * L10(f) - 0.6 * (hu - 1.5)
        else:
            pl_n = 35.3 * L10(d) + 22.4 + 21.3 * L10(f) - 0.3 * (hu - 1.5)
    elif scenario == "RMa":
        dbp = breakpoint_rma(fc, hb, hu)
        pl1, pl2 = rma_los_branches(d, f, dbp, h)
        pl_los = pl1 if d2 <= dbp else pl2
        pl_n = (161.04 - 7.1 * L10(w) + 7.5 * L10(h) - (24.37 - 3.7 * (h / hb) ** 2) * L10(hb) + (43.42 - 3.1 * L10(hb)) * (L10(d) - 3.0) + 20.0 * L10(f)
                - (3.2 * L10(11.75 * hu) ** 2 - 4.97))
    elif scenario == "InH":
        pl_los = 32.4 + 17.3 * L10(d) + 20.0 * L10(f)
        pl_n = 38.3 * L10(d) + 17.30 + 24.9 * L10(f)
    else:
        pl_los = 31.84 + 21.50 * L10(d) + 19.00 * L10(f)
        sl = 33.0 + 25.5 * L10(d) + 20.0 * L10(f)
        pl_n = {"InF-SL": sl, "InF-DL": max(18.6 + 35.7 * L10(d) + 20.0 * L10(f), sl), "InF-SH": 32.4 + 23.0 * L10(d) + 20.0 * L10(f),
                "InF-DH": 33.63 + 21.9 * L10(d) + 20.0 * L10(f), "InF-HH": pl_los}[scenario]
    return pl_los if los else max(pl_los, pl_n)


def fspl(fc, bs, ue):
    """fspl(R, lambda) of configFreeSpaceModel.m: 20 log10(4 pi R / lambda), negative values (and R = 0) -> 0."""
    r = math.sqrt(sum((float(a) - float(b)) ** 2 for a, b in zip(ue, bs)))
    if r == 0.0:
        return 0.0
    return max(20.0 * L10(4.0 * math.pi * r / (C0 / fc)), 0.0)


def thermal_noise_power(temperature_k, noise_figure_db, fs):
    """uePhy.m:945-947: Nt = k (T + 290 (10^(F/10) - 1)) fs."""
    return KB * (temperature_k + 290.0 * (10.0 ** (noise_figure_db / 10.0) - 1.0)) * fs


def dft_channel_matrix(nt, nr):
    """uePhy.m:735-737: H = fft(eye(n)); H = H(1:nt, 1:nr); H = H / norm(H)."""
    n = max(nt, nr)
    h = np.fft.fft(np.eye(n))[:nt, :nr]
    return h / np.linalg.norm(h, 2)


def rx_frontend(y, path_loss_db, rx_gain_db, noise_power, w=None):
    """uePhy.m:748, :938-939, :948-949: (db2mag(-pathLoss) y) 10^(RxGain/20) + sqrt(Nt/2) w   (w: unit randn + 1j randn, or None)."""
    s1, s2 = 10.0 ** (-path_loss_db / 20.0), 10.0 ** (rx_gain_db / 20.0)
    out = (np.asarray(y, dtype=np.complex128) * s1) * s2
    if w is not None:
        out = out + math.sqrt(noise_power / 2.0) * np.asarray(w, dtype=np.complex128)
    return out
