"""Physical scenes at every subcarrier spacing the library accepts (15 / 30 / 60 / 120 kHz): conftest.make_scene with the spacing as an argument, the table of eight scenes that
tests/test_numerology_cpu.py (oracle against the C++ port, no GPU) and tests/test_gpu_numerology.py (device against the oracle) share, and the oracle's results on them --
computed once per process, never written to.  Nothing here comes from the package under test.

Why the spacing matters (csrc/ofdm_symbol.hpp): the long cyclic prefix comes every 7 * 2^mu symbols and is cp_base + 16 (Nfft / 2048) 2^mu samples long, so symbol_start --
hence every demodulation window, the per-target beam windows and the slot offset inside a subframe -- differs from the 30 kHz layout wherever a scene crosses a half subframe.
At 60 and 120 kHz the scenes also reach what the 30 kHz ones hardly touch: target delays beyond the cyclic prefix (the table's `delay` against `cp`), so that echo samples of
the previous symbol lie inside the demodulation window."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import oracle as O

# symbol counts that end before, on and after each numerology's second long-CP symbol (symbol 7 * 2^mu), and -- where the CPI stays short -- after the third
LONG_CP_EDGES = {15: (1, 7, 8, 15), 30: (1, 14, 15, 29), 60: (1, 28, 29, 57), 120: (1, 56, 57)}

NEAR1 = ((150.0, 40.0, 1.5),)
PAIR = ((120.0, 60.0, 1.5), (-250.0, 80.0, 1.5))
SMALL = ((90.0, 20.0, 1.5),)


def scene(scs, nrb, n_ants, n_slots, targets, velocity, num_slots_param, zero_s_slots, seed=1, with_noise=True, nfft=None):
    """conftest.make_scene at the subcarrier spacing `scs` [kHz]: the same draw order (bits, then noise), nr_ofdm_info(nrb, scs), ofdm_modulate(grid, Nfft, scs), 'S' slots zeroed
    the same way; the same namespace.  `nfft` forces the carrier's transform length on both sides (waveform info and modulator) instead of nrOFDMInfo's choice."""
    ci = SimpleNamespace(NRBsDL=nrb, SubcarrierSpacing=scs)
    wi = O.nr_ofdm_info(nrb, scs)
    if nfft is not None:
        wi.Nfft, wi.SampleRate = int(nfft), float(nfft * scs * 1e3)
    cell = O.default_cell_params(n_ants=n_ants, target_pos=targets, velocity=velocity)
    if num_slots_param is not None:
        cell.numSlots = num_slots_param
    rp = O.radar_params(cell, ci, wi)
    rng = np.random.default_rng(seed)
    k, l = 12 * nrb, 14 * n_slots
    bits = rng.integers(0, 2, (2, k, l, n_ants)) * 2 - 1
    tx_grid = (bits[0] + 1j * bits[1]) / np.sqrt(2.0)
    if zero_s_slots:
        for s in range(3, n_slots, 4):
            tx_grid[:, 14 * s:14 * (s + 1), :] = 0
    amp = float(O.db2mag(cell.gNBTxPower - 30)) * np.sqrt(wi.Nfft ** 2 / (k * n_ants))
    tx_wave = O.ofdm_modulate(tx_grid, wi.Nfft, scs) * amp
    t = tx_wave.shape[0]
    noise = (rng.standard_normal((t, n_ants)) + 1j * rng.standard_normal((t, n_ants))) if with_noise else None
    return SimpleNamespace(cell=cell, carrier=ci, wave=wi, rp=rp, tx_grid=np.asfortranarray(tx_grid),
                           tx_wave=np.asfortranarray(tx_wave), noise=None if noise is None else np.asfortranarray(noise),
                           los=np.ones(len(targets), dtype=np.uint8), K=k, L=l, A=n_ants, T=t, amp=amp)


def _case(scs, nrb, n_ants, n_slots, num_slots_param, targets, velocity, zero_s_slots, nfft, n_fft, cp, delay):
    """`nfft`, `n_fft` (Doppler length), `cp` (normal, long) and `delay` (samples per target) are what the scene must come out with: asserted, not used to build it."""
    return SimpleNamespace(name=f"scs{scs}_nrb{nrb}_a{n_ants}", scs=scs, nrb=nrb, n_ants=n_ants, n_slots=n_slots, num_slots_param=num_slots_param, targets=targets,
                           velocity=velocity, zero_s_slots=zero_s_slots, nfft=nfft, L=14 * n_slots, n_fft=n_fft, cp=cp, delay=delay)


CASES = (
    _case(15, 24, 4, 4, 6, NEAR1, (0.0,), False, 512, 64, (36, 40), (9,)),
    _case(15, 52, 3, 4, 5, PAIR, (10.0, -6.0), True, 1024, 64, (72, 80), (15, 28)),
    _case(60, 24, 4, 4, 6, NEAR1, (0.0,), False, 512, 64, (36, 52), (33,)),
    _case(60, 66, 3, 8, 10, PAIR, (10.0, -6.0), True, 1024, 128, (72, 104), (57, 109)),
    _case(120, 24, 4, 8, 10, NEAR1, (0.0,), False, 512, 128, (36, 68), (65,)),
    _case(120, 66, 3, 8, 9, PAIR, (30.0, -20.0), True, 1024, 128, (72, 136), (113, 217)),
    _case(120, 11, 2, 4, 6, SMALL, (40.0,), False, 256, 64, (18, 34), (20,)),
    _case(60, 11, 2, 4, 6, SMALL, (15.0,), False, 256, 64, (18, 26), (10,)),
)
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)


def scene_of(case, **kw):
    return scene(case.scs, case.nrb, case.n_ants, case.n_slots, case.targets, case.velocity, case.num_slots_param, case.zero_s_slots, **kw)


def delays_of(rp):
    """ceil(pathDelay / Ts) per target (basicRadarChannel.m:21-22)."""
    return tuple(int(v) for v in np.ceil(2.0 * np.asarray(rp.range) / O.LIGHTSPEED * rp.fs))


def guard_margin(p_map, cut, pfa):
    """Smallest relative distance of a CUT cell's power from its CA-CFAR threshold: the number test_gpu_parity._guard_band_ok thresholds, returned rather than compared.  Above a
    bound it says that rounding-level differences in |rdm|^2 cannot flip a detection, so that detection lists may be compared exactly."""
    _, thr = O.ca_cfar2d(p_map, cut, pfa, return_threshold=True)
    pc = p_map[cut[0] - 1, cut[1] - 1]
    return float(np.min(np.abs(pc - thr) / np.maximum(np.abs(thr), 1e-300)))


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(float(np.abs(np.asarray(b)).max()), 1e-300))


_oracle = {}


def oracle_of(case):
    """namespace(sc, echo, est, dbg, cfg, margin [per antenna]) of a table case: the scene, the oracle's echo grid with the scene's time-domain noise, O.fft2d on it (rdm_explicit)
    and every antenna's guard margin.  Made once per process and shared; the arrays are read-only."""
    if case.name not in _oracle:
        sc = scene_of(case)
        echo = np.asfortranarray(O.mono_static_sensing(sc.tx_wave, sc.tx_grid.shape, sc.carrier, sc.rp, sc.los, sc.noise, nfft=sc.wave.Nfft))
        cfg = O.cfar2d_config(sc.rp)
        est, dbg = O.fft2d(sc.rp, cfg, echo, sc.tx_grid, return_debug=True, rdm_fn=O.rdm_explicit)
        margin = tuple(guard_margin(np.abs(dbg.rdm[:, :, a]) ** 2, cfg.CUTIdx, cfg.Pfa) for a in range(sc.A))
        for arr in (sc.tx_grid, sc.tx_wave, sc.noise, echo):
            arr.setflags(write=False)
        _oracle[case.name] = SimpleNamespace(sc=sc, echo=echo, est=est, dbg=dbg, cfg=cfg, margin=margin)
    return _oracle[case.name]


def lazy_cpi_case_120():
    """One lazy CPI at 120 kHz in tests/_lazy_cpi_reference.py's terms (Nfft = nIFFT = 4096, 49 antennas, two LoS targets, K = 1548): 57 symbols, one more than a half subframe, so
    the last column follows the numerology's second long prefix.  tests/test_numerology_cpu.py holds it a decade inside both suitability guards on the reference grid."""
    import _lazy_cpi_reference as R
    return R._case("k1548_a49_q2_scs120_57sym", 129, 49, (R.NEAR, R.MID), (10.0, -6.0), (1, 1), LONG_CP_EDGES[120][2], grid_seed=122, noise_seed=0x1C01, scs=120)
