"""CPI scenes at CFAR bands other than the default GuardBandSize = (2, 2), TrainingBandSize = (1, 1): the table that tests/test_cfar_band_cases_cpu.py (oracle alone, no GPU)
and tests/test_gpu_cfar_bands.py (device against the oracle) share, a restatement of the host rules that pick the kernels, and the oracle's results -- computed once per process,
never written to.  Nothing here comes from the package under test.

With the default bands hr = hc = 3 and gr = gc = 2, so a kernel that swaps the row and the column half sizes anywhere passes every default scene, and only a few sides of the
host's limits are ever reached.  The rules restated here (csrc/rdm.hip), with hr, hc = guard + training, gr, gc = guard, nr, nc = CUT rows, columns + 2 hr, 2 hc:

  panel detector (tail_fusable):  pr = 48 - 2 hr,  n_panels = ceil(n_cut_rows / pr);  taken when ALL of
        pr >= 8,  pr * n_cut_cols <= 2048,  n_panels <= 256,  n_cut_cols * n_panels <= 4096,  nc <= 128                       (LIMITS below, in this order)
  window detector (isac_cfar_window, every zone the panel detector leaves, and every zone of a context with tail fusion off):
        panel = floor(128 KiB / (8 nr)) - 2 hc CUT columns per pass;  panel < 1: the zone is refused (UNSUPPORTED)
  Doppler kernel:  nFFT != 256: doppler_pow_kernel;  nFFT = 256: the pruned doppler_fft256_kernel instantiation when every window column's bin (column - 129, 1-based column)
        lies in -16 .. 15, the full one otherwise.

Each case names the side of every limit it is meant to sit on; the CPU test proves it from the oracle's CUTIdx and holds every case to the 1e-9 decision margin that lets the GPU
tests compare integers exactly with nothing skipped.  The smallest margin over the table is 1.6e-05 (case dense_long_zone, 19 557 CUTs at Pfa = 0.5): MARGIN_FLOOR."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import oracle as O
from conftest import make_scene, spectral_to_time_noise
from oracle.fft2d import detect_per_antenna

LIMITS = ("pr", "pr_cols", "n_panels", "segments", "nc")
TAIL_ROWS = 48                    # window rows of one panel workgroup
LDS_BUDGET = 128 * 1024           # bytes of the window detector's staged columns
MARGIN = 1e-9                     # the suite's decision margin (test_gpu_parity._guard_band_ok)
MARGIN_FLOOR = 1.6e-5             # recorded: the smallest guard margin over the table (test_cfar_band_cases_cpu prints it and holds the table to it)

DEFAULT_BANDS = ((2, 2), (1, 1))
DEFAULT_ZONE = ((50.0, 500.0), (-50.0, 50.0))


# ------------------------------------------------------------------ the host rules, restated
def window_geometry(cut, guard, train):
    """CutWindow::of: the numbers of the CUT rectangle `cut` [2 x nCUT, 1-based] widened by guard + training cells."""
    row0, row1, col0, col1 = int(cut[0].min()), int(cut[0].max()), int(cut[1].min()), int(cut[1].max())
    gr, gc = (int(v) for v in guard)
    hr, hc = gr + int(train[0]), gc + int(train[1])
    n_cut_rows, n_cut_cols = row1 - row0 + 1, col1 - col0 + 1
    return SimpleNamespace(row0=row0, col0=col0, gr=gr, gc=gc, hr=hr, hc=hc, n_cut_rows=n_cut_rows, n_cut_cols=n_cut_cols, nr=n_cut_rows + 2 * hr, nc=n_cut_cols + 2 * hc,
                           first_row=row0 - hr, first_col=col0 - hc, n_train=(2 * hr + 1) * (2 * hc + 1) - (2 * gr + 1) * (2 * gc + 1))


def inside_map(g, n_ifft, n_fft):
    """All four sides: the window's first and last row / column are cells of the [nIFFT x nFFT] map (1-based)."""
    return g.first_row >= 1 and g.first_row + g.nr - 1 <= n_ifft and g.first_col >= 1 and g.first_col + g.nc - 1 <= n_fft


def panel_limits(g):
    """tail_fusable()'s five limits as {name: holds}; a panel below 8 rows is decided first (the others are then None: the host does not evaluate them)."""
    pr = TAIL_ROWS - 2 * g.hr
    if pr < 8:
        return dict(pr=False, pr_cols=None, n_panels=None, segments=None, nc=None), SimpleNamespace(pr=pr, n_panels=None)
    n_panels = -(-g.n_cut_rows // pr)
    return (dict(pr=True, pr_cols=pr * g.n_cut_cols <= 2048, n_panels=n_panels <= 256, segments=g.n_cut_cols * n_panels <= 4096, nc=g.nc <= 128),
            SimpleNamespace(pr=pr, n_panels=n_panels))


def window_panel(g):
    """isac_cfar_window's CUT columns per pass, before it is cut down to n_cut_cols; below 1 the zone is refused."""
    return LDS_BUDGET // (8 * g.nr) - 2 * g.hc


def detector_of(g, tail_fusion=True):
    """'panel' | 'window' | 'refused': what a context takes for the zone."""
    if tail_fusion and g.n_train > 0 and all(panel_limits(g)[0].values()):
        return "panel"
    return "window" if window_panel(g) >= 1 else "refused"


def doppler_kernel_of(g, n_fft):
    """'pow' | 'fft256_pruned' | 'fft256_full'."""
    if n_fft != 256:
        return "pow"
    bins = np.arange(g.first_col, g.first_col + g.nc) - 129          # CutWindow::velocity_of: bin 0 at column 129
    return "fft256_pruned" if bins.min() >= -16 and bins.max() <= 15 else "fft256_full"


def row_blocks(g):
    """The 512-row output blocks of the range transform that the window's rows touch, and those the CUT rows alone touch (0-based rows)."""
    return ((g.first_row - 1) // 512, (g.first_row + g.nr - 2) // 512), ((g.row0 - 1) // 512, (g.row0 + g.n_cut_rows - 2) // 512)


def guard_margin(p_map, cut, pfa, guard, train):
    """Smallest relative distance of a CUT cell's power from its CA-CFAR threshold at these bands."""
    _, thr = O.ca_cfar2d(p_map, cut, pfa, guard, train, return_threshold=True)
    pc = p_map[cut[0] - 1, cut[1] - 1]
    return float(np.min(np.abs(pc - thr) / np.maximum(np.abs(thr), 1e-300)))


def guard_band_ok(p_map, cut, pfa, guard, train, margin=MARGIN):
    """test_gpu_parity._guard_band_ok at the bands (guard, train): True when no CUT sits within `margin` (relative) of its threshold, so that rounding-level differences in
    |rdm|^2 cannot flip a detection."""
    _, thr = O.ca_cfar2d(p_map, cut, pfa, guard, train, return_threshold=True)
    pc = p_map[cut[0] - 1, cut[1] - 1]
    return bool(np.all(np.abs(pc - thr) > margin * np.maximum(np.abs(thr), 1e-300)))


# ------------------------------------------------------------------ the table
NEAR24 = ((150.0, 40.0, 1.5), (-90.0, 70.0, 5.0))      # 24 PRB: 158 and 117 m
FAR24 = ((400.0, 300.0, 1.5), (-700.0, 500.0, 5.0))    # 24 PRB: 501 and 861 m
NEAR273 = ((100.0, 20.0, 1.5), (250.0, -120.0, 1.5))   # 273 PRB: 106 and 279 m
LONG_ZONE = ((50.0, 2700.0), (-20.0, 20.0))            # 273 PRB: rows 42 .. 2214
TALL_ZONE = ((300.0, 1500.0), (-50.0, 50.0))           # 24 PRB: room for hr = 21 above the first CUT row


def _case(name, nrb, n_slots, num_slots_param, n_ants, targets, velocity, seed, detection_area, guard, train, pfa=None, *, n_fft, detector, doppler, unfused="window",
          limits=None, counts=None, kind="detect"):
    """`n_fft`, `detector` (with tail fusion on), `unfused` (with it off), `doppler`, `limits` ({limit: side it must sit on}) and `counts` (n_cut_rows, n_cut_cols, pr, n_panels,
    nc: whichever the case pins) are what the scene must come out with: asserted by the CPU test, not used to build it.  `kind`: 'detect' | 'quiet' | 'refused'."""
    return SimpleNamespace(name=name, nrb=nrb, n_slots=n_slots, num_slots_param=num_slots_param, n_ants=n_ants, targets=targets, velocity=velocity, seed=seed,
                           detection_area=detection_area, guard=tuple(guard), train=tuple(train), pfa=pfa, n_fft=n_fft, n_ifft=512 if nrb == 24 else 4096, detector=detector,
                           unfused=unfused, doppler=doppler, limits=dict(limits or {}), counts=dict(counts or {}), kind=kind)


# Where the guard is narrower than a target's main lobe the target raises its own threshold and the default Pfa = 1e-9 detects nothing: those band sets run at Pfa = 1e-2,
# where noise cells detect (the lists are then a few dozen cells long, spread over the zone)
ASYM_BANDS = (("g13_t21", (1, 3), (2, 1), None),       # hr = 3, hc = 4
              ("g31_t12", (3, 1), (1, 2), 1e-2),       # hr = 4, hc = 3
              ("g02_t11", (0, 2), (1, 1), 1e-2),       # no guard rows:     hr = 1, hc = 3
              ("g21_t02", (2, 1), (0, 2), 1e-2))       # no training rows:  hr = 2, hc = 3 (the guard rows are the window's outermost)

CASES = []
for _tag, _g, _t, _pfa in ASYM_BANDS:                  # every asymmetric band set on each Doppler kernel and both range transforms
    CASES.append(_case(f"nrb24_nfft64_{_tag}", 24, 6, 6, 2, NEAR24, (0.0, 6.0), 21, None, _g, _t, _pfa, n_fft=64, detector="panel", doppler="pow"))
    CASES.append(_case(f"nrb24_nfft256_{_tag}", 24, 6, None, 2, NEAR24, (0.0, 6.0), 22, None, _g, _t, _pfa, n_fft=256, detector="panel",
                       doppler="fft256_pruned" if _g[1] + _t[1] <= 4 else "fft256_full"))
    CASES.append(_case(f"nrb273_{_tag}", 273, 4, None, 2, NEAR273, (7.0, -4.0), 23, None, _g, _t, _pfa, n_fft=256, detector="panel", doppler="fft256_pruned"))
CASES += [
    # the two doppler_fft256_kernel instantiations: default zone = columns 118 .. 140 = bins -11 .. 11
    _case("hc4_pruned", 273, 4, None, 1, NEAR273, (7.0, -4.0), 31, None, (2, 2), (1, 2), n_fft=256, detector="panel", doppler="fft256_pruned", counts=dict(n_cut_cols=23)),
    _case("hc5_full", 273, 4, None, 1, NEAR273, (7.0, -4.0), 31, None, (2, 3), (1, 2), n_fft=256, detector="panel", doppler="fft256_full", counts=dict(n_cut_cols=23)),
    # panel height: hr = 20 -> pr = 8; hr = 21 -> pr = 6
    _case("pr8_panel", 24, 6, None, 2, FAR24, (0.0, 6.0), 41, TALL_ZONE, (4, 1), (16, 1), n_fft=256, detector="panel", doppler="fft256_pruned",
          limits=dict(pr=True), counts=dict(pr=8)),
    _case("pr6_window", 24, 6, None, 2, FAR24, (0.0, 6.0), 41, TALL_ZONE, (5, 1), (16, 2), n_fft=256, detector="window", doppler="fft256_pruned",
          limits=dict(pr=False), counts=dict(pr=6)),
    # pr * n_cut_cols: hr = 12 -> pr = 24; 85 columns = 2040, 86 columns = 2064
    _case("prcols_2040", 273, 4, None, 1, NEAR273, (7.0, -4.0), 51, ((50.0, 500.0), (-192.0, 192.0)), (2, 1), (10, 1), n_fft=256, detector="panel", doppler="fft256_full",
          limits=dict(pr_cols=True), counts=dict(pr=24, n_cut_cols=85)),
    _case("prcols_2064", 273, 4, None, 1, NEAR273, (7.0, -4.0), 51, ((50.0, 500.0), (-192.0, 196.0)), (2, 1), (10, 1), n_fft=256, detector="window", doppler="fft256_full",
          limits=dict(pr_cols=False), counts=dict(pr=24, n_cut_cols=86)),
    # nc through hc on one zone: 80 columns + 2 * 24 = 128, + 2 * 25 = 130
    _case("nc_128", 273, 4, None, 1, NEAR273, (7.0, -4.0), 52, ((60.0, 400.0), (-182.0, 178.0)), (2, 3), (10, 21), n_fft=256, detector="panel", doppler="fft256_full",
          limits=dict(nc=True), counts=dict(pr=24, n_cut_cols=80, nc=128)),
    _case("nc_130", 273, 4, None, 1, NEAR273, (7.0, -4.0), 52, ((60.0, 400.0), (-182.0, 178.0)), (2, 3), (10, 22), n_fft=256, detector="window", doppler="fft256_full",
          limits=dict(nc=False), counts=dict(pr=24, n_cut_cols=80, nc=130)),
    # n_panels: hr = 20 -> pr = 8; 2048 rows = 256 panels, 2049 rows = 257
    _case("panels_256", 273, 4, None, 1, NEAR273, (7.0, -4.0), 53, ((50.0, 2547.0), (-20.0, 20.0)), (3, 1), (17, 1), n_fft=256, detector="panel", doppler="fft256_pruned",
          limits=dict(n_panels=True), counts=dict(pr=8, n_cut_rows=2048, n_panels=256)),
    _case("panels_257", 273, 4, None, 1, NEAR273, (7.0, -4.0), 53, ((50.0, 2548.5), (-20.0, 20.0)), (3, 1), (17, 1), n_fft=256, detector="window", doppler="fft256_pruned",
          limits=dict(n_panels=False), counts=dict(pr=8, n_cut_rows=2049, n_panels=257)),
    # n_cut_cols * n_panels: 256 panels of 8 rows; 16 columns = 4096, 17 columns = 4352
    _case("segments_4096", 273, 4, None, 1, NEAR273, (7.0, -4.0), 54, ((50.0, 2547.0), (-36.0, 32.0)), (3, 0), (17, 2), n_fft=256, detector="panel", doppler="fft256_pruned",
          limits=dict(segments=True), counts=dict(pr=8, n_panels=256, n_cut_cols=16)),
    _case("segments_4352", 273, 4, None, 1, NEAR273, (7.0, -4.0), 54, ((50.0, 2547.0), (-36.0, 36.0)), (3, 0), (17, 2), n_fft=256, detector="window", doppler="fft256_pruned",
          limits=dict(segments=False), counts=dict(pr=8, n_panels=256, n_cut_cols=17)),
    # neither detector takes it: hr = 21 (no panel detector), 2215 window rows and hc = 4 -> 7 - 8 columns per pass
    _case("refused", 273, 4, None, 1, NEAR273, (7.0, -4.0), 55, LONG_ZONE, (5, 1), (16, 3), n_fft=256, detector="refused", unfused="refused", doppler="fft256_pruned",
          limits=dict(pr=False), kind="refused"),
    # dense lists (Pfa = 0.5): every (column, panel) segment of the merge non-empty; the second one's unfused context walks 5-column passes over 9 CUT columns
    _case("dense_default_zone", 273, 4, None, 2, NEAR273[:1], (7.0,), 61, None, (1, 3), (2, 1), 0.5, n_fft=256, detector="panel", doppler="fft256_pruned"),
    _case("dense_long_zone", 273, 4, None, 1, NEAR273[:1], (7.0,), 62, LONG_ZONE, (1, 0), (2, 1), 0.5, n_fft=256, detector="panel", doppler="fft256_pruned",
          counts=dict(n_cut_cols=9)),
    # nothing detected: no guard column, so the target's own Doppler main lobe lies in its training columns
    _case("quiet", 24, 6, None, 2, ((400.0, 0.0, 1.5),), (0.0,), 71, ((150.0, 1500.0), (-50.0, 50.0)), (3, 0), (1, 2), n_fft=256, detector="panel", doppler="fft256_pruned",
          kind="quiet"),
]
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)

# the routes that share the row window (cached range rows, the fused range stage).  hr = 12: CUT rows inside one 512-row block, the window's rows across two
RANGE_WINDOW_CASE = _case("range_window_two_blocks", 273, 4, None, 3, ((100.0, 20.0, 1.5),), (7.0,), 17, ((632.0, 1000.0), (-50.0, 50.0)), (2, 1), (10, 1), 0.5, n_fft=256,
                          detector="panel", doppler="fft256_pruned")
# (the readers of the last CPI's window -- re-detection, target lists, refinement, beam planes, cancellation -- run one scene at other bands in their own tests:
# tests/_target_list_restatement.py, READER_BANDS)


def scene_of(case):
    sc = make_scene(n_ants=case.n_ants, n_slots=case.n_slots, nrb=case.nrb, targets=case.targets, velocity=case.velocity, seed=case.seed,
                    detection_area=case.detection_area, num_slots_param=case.num_slots_param)
    if case.pfa is not None:
        sc.rp.Pfa = case.pfa
    return sc


def config_of(case, sc):
    """The oracle's detector configuration for the case: O.cfar2d_config with the case's bands."""
    ocf = O.cfar2d_config(sc.rp)
    ocf.GuardBandSize, ocf.TrainingBandSize = case.guard, case.train
    return ocf


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(float(np.abs(np.asarray(b)).max()), 1e-300))


def chain_on(sc, cfg, echo, rdm=None):
    """O.fft2d (rdm_explicit) on an echo grid at the configuration `cfg` -> namespace(sc, echo, cfg, geom, est | None, dbg, margin [per antenna])."""
    guard, train = cfg.GuardBandSize, cfg.TrainingBandSize
    if rdm is None:
        rdm = O.rdm_explicit(echo, sc.tx_grid, int(sc.rp.nIFFT), int(sc.rp.nFFT))
        rdm.setflags(write=False)
    try:
        est, dbg = O.fft2d(sc.rp, cfg, echo, sc.tx_grid, return_debug=True, rdm_fn=lambda *a: rdm)
    except ValueError:
        dets, _, _ = detect_per_antenna(rdm, cfg, sc.rp.rRes, sc.rp.vRes, int(sc.rp.nFFT))
        est, dbg = None, SimpleNamespace(rdm=rdm, detections=dets, Ra=O.covariance(echo))
    margin = tuple(guard_margin(np.abs(rdm[:, :, a]) ** 2, cfg.CUTIdx, cfg.Pfa, guard, train) for a in range(sc.A))
    return SimpleNamespace(sc=sc, echo=echo, cfg=cfg, geom=window_geometry(cfg.CUTIdx, guard, train), est=est, dbg=dbg, margin=margin)


_oracle = {}


def oracle_of(case, default_bands=False):
    """chain_on the case's scene and the oracle's echo grid (the scene's time-domain noise) at the case's bands (est is None where the oracle detects nothing).
    `default_bands`: the same scene, zone and Pfa at GuardBandSize = (2, 2), TrainingBandSize = (1, 1).  Made once per process and shared; the arrays are read-only."""
    key = (case.name, default_bands)
    if key not in _oracle:
        if default_bands:
            base = oracle_of(case)
            _oracle[key] = chain_on(base.sc, O.cfar2d_config(base.sc.rp), base.echo, base.dbg.rdm)
        else:
            sc = scene_of(case)
            echo = np.asfortranarray(O.mono_static_sensing(sc.tx_wave, sc.tx_grid.shape, sc.carrier, sc.rp, sc.los, sc.noise, nfft=sc.wave.Nfft))
            for arr in (sc.tx_grid, sc.tx_wave, sc.noise, echo):
                arr.setflags(write=False)
            _oracle[key] = chain_on(sc, config_of(case, sc), echo)
    return _oracle[key]


# the scenes that tests/test_gpu_cfar_bands.py also runs at the default bands (after the refused call; inside the context-reuse sequence)
DEFAULT_BAND_RERUNS = ("refused", "pr8_panel")

SPECTRAL_SEED = 5


def spectral_reference_of(case, seed=SPECTRAL_SEED):
    """chain_on the case's scene with the library's seeded spectral noise restated (oracle/philox.py) and mapped back to the oracle's time-domain AWGN: the grid that
    monoStaticSensing(seed=seed, noise_domain="spectral") forms to within the float32 Box-Muller's 1e-7 of the noise level.  The CPU test holds its guard margin three decades
    above that; the GPU test takes the oracle on the grid the device materialised."""
    key = (case.name, "spectral", seed)
    if key not in _oracle:
        sc = oracle_of(case).sc
        w = O.philox_spectral_noise(sc.K, sc.L, sc.A, seed)
        tnoise = spectral_to_time_noise(w, sc.T, sc.wave.Nfft, sc.carrier.SubcarrierSpacing, sc.rp.fc, sc.rp.fs)
        echo = np.asfortranarray(O.mono_static_sensing(sc.tx_wave, sc.tx_grid.shape, sc.carrier, sc.rp, sc.los, tnoise, nfft=sc.wave.Nfft))
        _oracle[key] = chain_on(sc, config_of(case, sc), echo)
    return _oracle[key]
