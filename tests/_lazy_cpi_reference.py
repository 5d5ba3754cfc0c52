"""An fp64 NumPy reference of the LAZY CPI (isac_mono_static_sensing_fused_dev with d_echo_grid == NULL on the spectral Philox route: echo_range_sl_kernel<Q, 1, false>,
cov_lazy_kernel<Q>, the one-launch beam-sum), written from the oracle alone -- nothing here comes from the package under test or from a device:

  * `build_scene`: test_gpu_valu_diet._scene's recipe (Nfft = nIFFT = 4096 at every K; nrOFDMInfo would pick less below 3276 subcarriers) returning the oracle's
    radar_params and, where the caller hands in the library's radarParams function, the library's -- both from ONE cell / carrier / waveform description and with the same
    overrides (nIFFT = 4096, rRes), so that O.fft2d and the library see one parameter set; the subcarrier spacing is the case's (`scs`: 30 kHz for the whole table,
    120 kHz for the one case of tests/test_gpu_numerology.py);
  * `reference_echo`: O.mono_static_sensing (the per-antenna time-domain chain, monoStaticSensing.m:1-23) fed the time-domain noise that demodulates to the restated Philox
    field (oracle/philox.py), zero-padded to L_out by the oracle itself;
  * `reference_covariance`: Ra = G^H G / (K L_out) (fft2D.m:106-107) and the per-antenna mean magnitudes of the element-error bound;
  * `oracle_chain`: O.fft2d on a grid, with the two input-suitability margins (CFAR threshold distance, eigenvalue gap at the signal / noise split) from the oracle's numbers;
  * `s_col` / `staged_grid` / `slab_plan`: csrc/cov.hip's slab arithmetic restated, used ONLY to assert that the shape table reaches the cases it is there for -- never as an
    expected value for the device.

The Philox field of a zero-padded grid (L_out > L_whole): the generator's counter is (slot + 2048 column) with column = l + n_sym a on the grid AS STORED, [K x L_out x A]
(include/isac.h: the spectral fields are [n_sc x L_out x A]; oracle/philox.py: W [n_sc x n_sym x n_ants]) -- the reference draws the L_out-column field and keeps its first
L_whole columns; the padding columns carry neither echo nor noise (monoStaticSensing.m:19-21)."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import oracle as O
from conftest import spectral_to_time_noise

NFFT = 4096
SCS_KHZ = 30
LIGHTSPEED = 299792458.0
NEAR, MID, FAR = (100.0, 20.0, 1.5), (-250.0, 80.0, 1.5), (470.0, 60.0, 1.5)      # test_gpu_valu_diet.py: delay shifts 86, 216, 390 samples; CP = 288 / 352 samples
RTOL = 1e-10                                                                      # test_gpu_fullsize.RTOL


DEFAULT_BANDS = ((2, 2), (1, 1))                                                  # cfar2D.m:32-33: GuardBandSize, TrainingBandSize


def _case(name, nrb, n_ants, targets, velocity, los, n_sym, cut=0, silent=(), zero_from=None, grid_seed=1, noise_seed=1, pfa=1e-9, rcs=1.0, scs=SCS_KHZ, bands=DEFAULT_BANDS):
    return SimpleNamespace(name=name, nrb=nrb, n_ants=n_ants, targets=tuple(targets), velocity=tuple(velocity), los=tuple(los), n_sym=n_sym, cut=cut,
                           silent=tuple(silent), zero_from=zero_from, grid_seed=grid_seed, noise_seed=noise_seed, pfa=pfa, rcs=rcs, scs=scs,
                           bands=(tuple(bands[0]), tuple(bands[1])))


# `cut`: samples dropped from the waveform's end (the last symbol becomes incomplete: L_whole = L_out - 1); `silent`: transmit-silent columns (txGrid zero: rx .* conj(0));
# `zero_from`: the columns from here on are a zero-filled 'S' slot (gNBPhy.m:609-612).  Seeds: chosen on the CPU (tests/test_lazy_cpi_reference_cpu.py) so that both guards of
# oracle_chain hold with a decade to spare.
TABLE = (
    _case("k288_a64", 24, 64, (NEAR,), (7.0,), (1,), 14, grid_seed=101, noise_seed=0x1A01),
    _case("k516_a49", 43, 49, (MID,), (-6.0,), (1,), 14, grid_seed=102, noise_seed=0x1A02),
    _case("k1020_a63_q2", 85, 63, (NEAR, MID), (10.0, -6.0), (1, 1), 14, grid_seed=103, noise_seed=0x1A03, pfa=1e-5),
    _case("k1032_a64_13of14", 86, 64, (NEAR,), (7.0,), (1,), 14, cut=3000, grid_seed=104, noise_seed=0x1A04, pfa=1e-5),
    _case("k1032_a56_q2_27of28", 86, 56, (NEAR, MID), (10.0, -6.0), (1, 1), 28, cut=3000, silent=(5,), grid_seed=105, noise_seed=0x1A05, pfa=1e-5),
    _case("k1548_a64_blocked_between", 129, 64, ((120.0, 60.0, 1.5), (60.0, -30.0, 1.5), (-250.0, 80.0, 1.5)), (10.0, 3.0, -6.0), (1, 0, 1), 14, grid_seed=106, noise_seed=0x1A06),
    _case("k3276_a64_first_blocked", 273, 64, (MID, NEAR), (-6.0, 7.0), (0, 1), 14, grid_seed=107, noise_seed=0x1A07, rcs=1e-2),
    _case("k3276_a50_q2_s_slot", 273, 50, (NEAR, FAR), (7.0, 3.0), (1, 1), 28, zero_from=14, grid_seed=108, noise_seed=0x1A08),
)
# the two antenna counts next to the 49..64 switch: the lazy entry point keeps the grid in a context-owned buffer there (csrc/echo.hip: lazy_native)
NEIGHBOURS = (
    _case("k516_a48_owned", 43, 48, (MID,), (-6.0,), (1,), 14, grid_seed=111, noise_seed=0x1B01),
    _case("k516_a65_owned", 43, 65, (MID,), (-6.0,), (1,), 14, grid_seed=112, noise_seed=0x1B02),
)
# one CPI at other guard / training bands than the default, at the smallest shape the lazy tests use (tests/test_gpu_range_dead_columns.py: 25 PRB, 49 antennas, one target):
# hr = 16 != hc = 4 and gr = 10 != gc = 1 -- the row window the lazy range kernel takes (CutRows) and the Doppler kernel's col_lo / nc differ from every other lazy case's.
# The ten guard rows step over the range main lobe, which is what lets a K = 300 scene detect at all; RCS = 1e-4 keeps the eigenvalue gap at the signal / noise split three
# decades above its guard (tests/test_lazy_cpi_reference_cpu.py)
BAND_CASE = _case("k300_a49_bands_g10_1_t6_3", 25, 49, (NEAR,), (7.0,), (1,), 14, grid_seed=131, noise_seed=0x1D01, rcs=1e-4, bands=((10, 1), (6, 3)))
SWEEP_SEEDS = (9001, 9008, 9009, 9019, 9032, 9034)
SWEEP_NRB = (24, 43, 86, 129, 273)
SWEEP_RCS = 1e-2


def pfa_for(nrb):
    return 1e-5 if nrb in (85, 86) else 1e-9


def sweep_case(seed):
    """One seeded scene of the sweep: nrb from SWEEP_NRB, 49..64 antennas, one or two targets at random positions and velocities inside the detection area (radar.m:10: 50..500 m,
    +-50 m/s), LoS flags random with at least one set, one slot."""
    rng = np.random.default_rng(seed)
    nrb = int(rng.choice(SWEEP_NRB))
    n_ants = int(rng.integers(49, 65))
    q = int(rng.integers(1, 3))
    r = rng.uniform(70.0, 450.0, q)                                        # ground distance [m]: slant range sqrt(r^2 + 28.5^2) stays inside 50..500 m
    az = rng.uniform(-np.pi, np.pi, q)
    targets = tuple((float(r[i] * np.cos(az[i])), float(r[i] * np.sin(az[i])), 1.5) for i in range(q))
    velocity = tuple(float(v) for v in rng.uniform(-45.0, 45.0, q))
    los = rng.integers(0, 2, q)
    if not los.any():
        los[int(rng.integers(0, q))] = 1
    return _case(f"sweep{seed}", nrb, n_ants, targets, velocity, tuple(int(v) for v in los), 14, grid_seed=seed, noise_seed=0x5EED0000 + seed, pfa=pfa_for(nrb), rcs=SWEEP_RCS)


# ---------------------------------------------------------------- csrc/cov.hip's slab arithmetic, restated (coverage assertions only)
def s_col(k):
    """Slabs per symbol column (isac_covariance_lazy_on): 8 pair rows (k, k + 512) per slab, one 1024-subcarrier block pair after the other."""
    return sum((min(512, k - k0) + 7) // 8 for k0 in range(0, k, 1024))


def staged_grid(slabs):
    """cov_staged_grid: at most 512 workgroups, `per` slabs each, `per` rounded up to even -> (workgroups, per)."""
    gx = min(512, slabs)
    per = -(-slabs // gx)
    per = (per + 1) & ~1
    return -(-slabs // per), per


def slab_plan(case):
    k = 12 * case.nrb
    l_whole = case.n_sym - (1 if case.cut else 0)
    sc = s_col(k)
    slabs = l_whole * sc
    gx, per = staged_grid(slabs)
    tail = k % 1024                                                        # rows of the last block pair; its partner half holds max(0, tail - 512) of them (tail = 0: a whole pair)
    partner = 512 if tail == 0 else max(0, tail - 512)
    return SimpleNamespace(K=k, L_whole=l_whole, L_out=case.n_sym, s_col=sc, slabs=slabs, gx=gx, per=per, last=slabs - (gx - 1) * per, partner_rows=partner,
                           partner_ends_inside_slab=partner % 8 != 0, masked_antennas=64 - case.n_ants if 48 < case.n_ants <= 64 else 0)


# ---------------------------------------------------------------- scene
def build_scene(case, lib_radar_params=None):
    """QPSK txGrid on every antenna plane, CP-OFDM waveform at Nfft = 4096 scaled by signalAmp (gNBPhy.m:592), the oracle's radar_params (`orp`) and -- with the library's
    radarParams function handed in -- the library's (`rp`), both with nIFFT = 4096 and the rRes that goes with it (radarParams.m:69,71)."""
    scs = case.scs                                                         # [kHz]; the table's cases are at SCS_KHZ
    ci = SimpleNamespace(NRBsDL=case.nrb, SubcarrierSpacing=scs)
    wi = SimpleNamespace(Nfft=NFFT, SampleRate=NFFT * scs * 1e3, SymbolsPerSlot=14, SlotsPerSubframe=scs // 15)
    cell = O.default_cell_params(n_ants=case.n_ants, target_pos=case.targets, velocity=case.velocity, rcs=np.full(len(case.targets), case.rcs))
    # the CPI is one or two slots: numSlots (radarParams.m:18-21,75) says so, nFFT = 32 / 64 -- with the default 20 the 14 live symbols sit in a 256-point Doppler transform
    # whose main lobe covers the CFAR training ring, and no scene of the table could have a detection (test_gpu_spectral._range_stage_scene does the same)
    cell.numSlots = 2 * (case.n_sym // 14)
    cell.Pfa = case.pfa
    rng = np.random.default_rng(case.grid_seed)
    k, a = 12 * case.nrb, case.n_ants
    bits = rng.integers(0, 2, (2, k, case.n_sym, a)) * 2 - 1
    tx_grid = np.asfortranarray((bits[0] + 1j * bits[1]) / np.sqrt(2.0))
    for col in case.silent:
        tx_grid[:, col, :] = 0
    if case.zero_from is not None:
        tx_grid[:, case.zero_from:, :] = 0
    amp = float(O.db2mag(cell.gNBTxPower - 30)) * np.sqrt(NFFT ** 2 / (k * a))
    tx_wave = O.ofdm_modulate(tx_grid, NFFT, scs) * amp
    tx_wave = np.asfortranarray(tx_wave[:tx_wave.shape[0] - case.cut])

    def overridden(fn):
        p = fn(cell, ci, wi)
        p.nIFFT = NFFT
        p.rRes = LIGHTSPEED / (2 * scs * 1e3 * p.nIFFT)
        return p

    starts, cps = O.symbol_starts(NFFT, scs, case.n_sym)
    l_whole = int(sum(int(starts[s]) + int(cps[s]) + NFFT <= tx_wave.shape[0] for s in range(case.n_sym)))
    for arr in (tx_grid, tx_wave):
        arr.setflags(write=False)
    return SimpleNamespace(case=case, cell=cell, carrier=ci, wave=wi, orp=overridden(O.radar_params), rp=None if lib_radar_params is None else overridden(lib_radar_params),
                           overridden=overridden, tx_grid=tx_grid, tx_wave=tx_wave, los=np.asarray(case.los, dtype=np.uint8), K=k, A=a, T=tx_wave.shape[0], L_out=case.n_sym, L_whole=l_whole)


def noise_sigma(sc):
    """Standard deviation of the real / imaginary part of the spectral noise on the demodulated grid (include/isac.h, isac_noise_mode: CN(0, Nfft N0))."""
    return float(np.sqrt(sc.orp.N0 / 2.0) * np.sqrt(NFFT))


# ---------------------------------------------------------------- reference echo grid and covariance
def reference_echo(sc, with_noise=True):
    """echoGrid [K x L_out x A] of the oracle's time-domain chain; the noise is the restated Philox field of the stored grid, mapped back to the time domain."""
    tnoise = None
    if with_noise:
        w = O.philox_spectral_noise(sc.K, sc.L_out, sc.A, sc.case.noise_seed)[:, :sc.L_whole, :]
        tnoise = spectral_to_time_noise(w, sc.T, NFFT, sc.case.scs, sc.orp.fc, sc.orp.fs)
    e = O.mono_static_sensing(sc.tx_wave, (sc.K, sc.L_out, sc.A), sc.carrier, sc.orp, sc.los, tnoise, nfft=NFFT)
    e = np.asfortranarray(e)
    e.setflags(write=False)
    return e


def reference_covariance(e):
    """(Ra, m): Ra = G^H G / (K L_out), G = reshape(E, K L_out, A) (fft2D.m:106-107); m[a] = mean_n |G[n, a]|."""
    k, l, a = e.shape
    g = e.reshape(k * l, a, order="F")
    return (g.conj().T @ g) / (k * l), np.abs(g).mean(axis=0)


def echo_bound(sc, e):
    """eta: float32 hardware Box-Muller against its float32 restatement on a unit sample, scaled, plus the 1e-10 of the fp64 chains (test_gpu_spectral.py)."""
    return noise_sigma(sc) * O.philox.SPECTRAL_NOISE_ATOL + RTOL * float(np.abs(e).max())


def covariance_bound(eta, m, ra_ref):
    """|sum_n conj(x + dx)(y + dy) - conj(x) y| / N <= eta (mean|x| + mean|y|) + eta^2 for |dx|, |dy| <= eta; + the summation-order allowance of test_covariance_mfma."""
    return eta * (m[:, None] + m[None, :]) + eta * eta + 1e-12 * float(np.abs(ra_ref).max())


# ---------------------------------------------------------------- the oracle's fft2D on a grid, with the suitability margins
def cfar_config(sc):
    """O.cfar2d_config(orp) at the case's bands (the default ones for every case that does not name others)."""
    ocf = O.cfar2d_config(sc.orp)
    ocf.GuardBandSize, ocf.TrainingBandSize = sc.case.bands
    return ocf


def oracle_chain(sc, grid):
    """O.fft2d(orp, cfar_config(sc), grid, txGrid) with rdm_explicit -> namespace(est | None, rdm, detections, Ra, n_det, cfar_margin, eig_gap).
    cfar_margin: smallest relative distance of a CUT cell's power from its threshold, over every antenna; eig_gap: (w[L-1] - w[L]) / w[0] at the signal / noise split
    L = numel(rngEst) of the descending eigenvalues (inf where there is no split: no detection, or L >= A)."""
    ocf = cfar_config(sc)
    guard, train = ocf.GuardBandSize, ocf.TrainingBandSize
    keep = {}

    def rdm_fn(*args):
        keep["rdm"] = O.rdm_explicit(*args)
        return keep["rdm"]

    try:
        est, dbg = O.fft2d(sc.orp, ocf, grid, sc.tx_grid, return_debug=True, rdm_fn=rdm_fn)
        rdm, dets, ra = dbg.rdm, dbg.detections, dbg.Ra
    except ValueError:                                                     # findpeaks with NPeaks = 0 (music.m:102): no CUT detected
        est, rdm, ra = None, keep["rdm"], O.covariance(grid)
        dets = [O.ca_cfar2d(np.abs(rdm[:, :, a]) ** 2, ocf.CUTIdx, ocf.Pfa, guard, train) for a in range(sc.A)]
        assert not any(d.shape[1] for d in dets)
    margin = np.inf
    for a in range(sc.A):
        p = np.abs(rdm[:, :, a]) ** 2
        _, thr = O.ca_cfar2d(p, ocf.CUTIdx, ocf.Pfa, guard, train, return_threshold=True)
        pc = p[ocf.CUTIdx[0] - 1, ocf.CUTIdx[1] - 1]
        margin = min(margin, float(np.min(np.abs(pc - thr) / np.maximum(np.abs(thr), 1e-300))))
    gap = np.inf
    if est is not None:
        w = np.sort(np.linalg.eigvalsh(ra))[::-1]
        ls = int(est.rngEst.size)
        if 1 <= ls < sc.A:
            gap = float((w[ls - 1] - w[ls]) / w[0])
    return SimpleNamespace(est=est, cfg=ocf, rdm=rdm, detections=dets, Ra=ra, n_det=int(sum(d.shape[1] for d in dets)), cfar_margin=margin, eig_gap=gap)


_cache = {}


def reference_of(case, lib_radar_params=None):
    """(scene, E, Ra_ref, m, eta) of a case: made once per process, shared by the tests that need it, never written to."""
    if case.name not in _cache:
        sc = build_scene(case, lib_radar_params)
        e = reference_echo(sc)
        ra, m = reference_covariance(e)
        _cache[case.name] = (sc, e, ra, m, echo_bound(sc, e))
    sc = _cache[case.name][0]
    if sc.rp is None and lib_radar_params is not None:
        sc.rp = sc.overridden(lib_radar_params)
    return _cache[case.name]
