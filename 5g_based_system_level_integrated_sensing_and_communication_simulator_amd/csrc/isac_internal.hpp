// The interface between the translation units of libisac_hip: every function that one .hip file defines and another calls is declared here, once (default arguments
// included), and every .hip file includes this header -- the defining unit too, so the compiler sees both.  extern "C" entry points: include/isac.h, not here.
#pragma once
#include "isac_common.hpp"
#include "eigh_layout.hpp"
#include "beam_window.hpp"
#include "cpi_post.hpp"

// ---------------------------------------------------------------- tables.hip: cached device tables
// The one way a cached table comes to exist: `key` is looked up in ctx->tables; on a miss `build` fills a std::vector<T> on the host, which is uploaded and kept under
// the key until the context goes.  *out: the device pointer.
template <typename T, typename Build>
int cached_table(isac_ctx* ctx, const isac::TableKey& key, const T** out, Build build) {
  auto it = ctx->tables.find(key);
  if (it == ctx->tables.end()) {
    std::vector<T> v;
    build(v);
    isac::DevBuf b;
    ISAC_TRY(isac::upload(ctx, b, v.data(), sizeof(T) * v.size()));
    it = ctx->tables.emplace(key, std::move(b)).first;
  }
  *out = (const T*)it->second.p;
  return ISAC_OK;
}
int isac_get_twiddles(isac_ctx* ctx, int n, const isac::c64** out);
int isac_get_w512_pack(isac_ctx* ctx, const isac::c64** out);
int isac_get_logtab(isac_ctx* ctx, const isac::c64** out);
int isac_get_rise_window(isac_ctx* ctx, int n_win, const double** out);
int isac_get_windows(isac_ctx* ctx, int K, int n_ifft, const double** win_k, const double** win_r);
// ---------------------------------------------------------------- rdm.hip
int isac_rdm_power_window(isac_ctx* ctx, const isac_est_params* ep, const isac_cfar_config* cf, const isac::c64* d_rx, const isac::c64* d_tx, int K, int L, int A, bool use_cached_range);   // leaves the window of isac::CutWindow::of(*cf) in ctx->pwin
int check_rdm_dims(isac_ctx* ctx, const isac_est_params* ep, int K, int L, int A);   // ISAC_ERR_INVALID_ARG unless K, L, A > 0 and nIFFT >= K, nFFT > 0 are powers of two: what every entry that runs the range or the Doppler stage asks of its grids
int isac_cfar_window(isac_ctx* ctx, const isac_est_params* ep, const isac_cfar_config* cf, int A, int cap);
double cfar_alpha(int n_train, double pfa);   // CA, ThresholdFactor 'Auto': N (Pfa^(-1/N) - 1)
namespace isac { struct CutRows { int row_lo, nr; }; }   // rows [row_lo, row_lo + nr) of the range-Doppler map (0-based): the CUT rows +- (guard + training)
bool cut_rows_ok(const isac_est_params* ep, const isac_cfar_config* cf, isac::CutRows* out);              // false: the window leaves the map
int cut_rows(isac_ctx* ctx, const isac_est_params* ep, const isac_cfar_config* cf, isac::CutRows* out);   // ... as ISAC_ERR_CFAR_WINDOW
int isac_range_stage_into_cache(isac_ctx* ctx, const isac_est_params* ep, const isac_cfar_config* cf, const isac::c64* d_rx, const isac::c64* d_tx, int K, int L, int A);
// ---------------------------------------------------------------- targets.hip: isac_fft2d_get_targets (include/isac_targets.h) and isac_fft2d_get_targets_upa (include/isac_targets_upa.h) -- the per-target
// list of the last completed fft2D.  It calls nothing but isac_get_twiddles and (UPA) isac_doa2d_grid; beams.hip calls its target_cells_of_planes (below).  What it shares with the
// other units is ctx->tgt (isac::Fft2dCpi, isac_common.hpp): fft2d.hip fills it, rdm.hip / echo.hip drop it.
// ---------------------------------------------------------------- cfar.hip: the GOCA / SOCA / OS detectors (include/isac_cfar.h): isac_cfar2d, isac_fft2d_redetect, isac_cfar_threshold_factor.  Reads ctx->tgt and
// ctx->pwin, writes ctx->redet only; calls cfar_alpha (rdm.hip) and fft2d_estimates (fft2d.hip).  cfar_detect_planes (below) is its device half, shared with beams.hip.  Also isac_cfar_monte_carlo (include/isac_cfar_mc.h): reads nothing of the
// context, writes ctx->cfar_mc only.
// the detector of isac_fft2d_redetect on any planes with the power window's geometry (callers: isac_fft2d_redetect, isac_fft2d_beam_detect): per-plane CUT-order lists in `scratch`
namespace isac {
struct PlaneLists {
  int n_planes = 0, n_cut = 0;             // every plane's list has room for all n_cut CUTs: plane a at d_cut + a n_cut, d_pow + a n_cut
  const double* d_pow = nullptr; const int* d_cut = nullptr; const int* d_cnt = nullptr;   // device: the CUTs' powers, CUT ordinals, counts [n_planes]
  std::vector<int> off;                    // host [n_planes + 1]: offsets of the concatenated lists
  int rows_seen = 0;                       // distinct CUT rows with a detection (numDets)
  int total() const { return off.empty() ? 0 : off.back(); }
};
}
int cfar_detect_planes(isac_ctx* ctx, const char* who, const isac_cfar_method* m, const double* d_planes, int n_planes, isac::DevBuf& scratch, isac::PlaneLists* pl);
int cfar_fetch_lists(isac_ctx* ctx, const isac::PlaneLists& pl, std::vector<int>& cut, std::vector<double>& pw);
// ... and its first kernel alone, for beam_clean.hip: the per-CUT flags [n_planes][n_cut] of the CUT rows [cut_row_lo, cut_row_hi) (0-based inside the zone, clipped to it)
// into d_flags, the other rows' flags untouched; an empty range checks the method block and the detector's limits and launches nothing
int cfar_flag_planes(isac_ctx* ctx, const char* who, const isac_cfar_method* m, const double* d_planes, int n_planes, int cut_row_lo, int cut_row_hi, unsigned char* d_flags);
// ---------------------------------------------------------------- targets.hip, for beams.hip: steps 1, 2 and 5 of the lists (hits, local maxima of the map, order, every field of *out but azi and n_targets) on the
// planes [nr x nc x n_planes] and per-plane lists of `src`
namespace isac {
struct PlaneCells {
  const double* planes; int n_planes;
  const int* det_cut; const int* det_cnt; int cap;   // device: CUT ordinals [n_planes x cap], counts [n_planes]
  bool take_max;                           // false: the map is the sum over the planes; true: their maximum, and best_plane[i] (host, [ISAC_MAX_TARGETS], 0-based) its first plane
  DevBuf* scratch;
  int32_t* best_plane;
};
}
int target_cells_of_planes(isac_ctx* ctx, const char* who, const isac::PlaneCells& src, isac_target_list* out);
// ... and for refine.hip: step 4 (ULA) / 4' (UPA, by ctx->tgt.ep) of the lists on n snapshots [A x n] that are on the device: the scan bins into d_bin [n], azi [n] (and ele [n],
// UPA only) on the host; complete when it returns.  UPA: the checks of isac_doa2d_grid; the scan's partials go to ctx->tgt_part.
int target_scan_snapshots(isac_ctx* ctx, const isac::c64* d_snap, int n, int* d_bin, double* azi, double* ele);
// ---------------------------------------------------------------- refine.hip: isac_fft2d_refine_targets (include/isac_refine.h) -- off-grid Doppler, split-lobe merge and sidelobe flags for listed cells of the
// last completed fft2D.  Reads ctx->tgt and ctx->ymid, writes ctx->refine (and ctx->tgt_part through target_scan_snapshots) only.
// For clean.hip and relax.hip: steps 1-3 of isac_refine.h on n cells of the range rows d_rows [nr x L x A] (ctx->ymid, or a residual copy of it): tone_plan sizes the probes
// for the CPI (ISAC_ERR_UNSUPPORTED: they do not fit the LDS) and, for a planar array, runs the checks of isac_doa2d_grid that target_scan_snapshots would meet only after
// the work (n_ants_x n_ants_y != A: ISAC_ERR_INVALID_ARG; A > 256: ISAC_ERR_UNSUPPORTED); refine_enqueue launches refine_kernel on the context's stream.  d_cell_row: window
// rows, 0-based; d_cell_k: col - nFFT/2 - 1.
namespace isac { struct RefinePlan { double W = 0.0; int M = 0; size_t lds = 0; }; }
int tone_plan(isac_ctx* ctx, const char* who, isac::RefinePlan* plan);
int refine_enqueue(isac_ctx* ctx, const isac::RefinePlan& plan, const isac::c64* d_rows, const int* d_cell_row, const int* d_cell_k, int n, int* d_status, double* d_nu, double* d_pow, isac::c64* d_snap /* [A x n] */);
// ---------------------------------------------------------------- beams.hip: isac_fft2d_get_rdm_window, isac_fft2d_beam_detect (include/isac_beams.h) -- the complex window of the last completed fft2D and CFAR on
// beam planes of it.  Reads ctx->tgt and ctx->ymid, writes ctx->beam_y / beam_p / beam_det / beam_sel only; calls isac_get_twiddles, cfar_detect_planes and target_cells_of_planes.
// What every call on "the last completed fft2D" asks first (the rule of isac_fft2d_get_targets): a completed fft2D whose range rows are still the ones it left, else
// ISAC_ERR_INVALID_ARG; and what every local-maximum test asks of the CFAR window: a halo of at least one cell in both dimensions, else ISAC_ERR_UNSUPPORTED.  who: the
// entry point, for the message.
int cpi_ready(isac_ctx* ctx, const char* who);
int needs_halo(isac_ctx* ctx, const char* who);
// For clean.hip and beam_clean.hip: step 1 of isac_beams.h: rdm_window_kernel on the range rows d_rows [nr x L x A] into d_Y [nr x nc x A] (both sized by the caller), enqueued on the context's stream
int rdm_window_enqueue(isac_ctx* ctx, const char* who, const isac::c64* d_rows, isac::c64* d_Y);
// For beam_clean.hip: n_b of every column of the host weights W [A x B] (ISAC_ERR_INVALID_ARG: a zero or non-finite norm), and step 2 of isac_beams.h: beam_planes_kernel on
// d_Y [n_cells x A] with the weights d_W [A x B] and norms d_norm [B] into d_Pb [n_cells x B] (all on the device, sized by the caller), enqueued on the context's stream
int beam_weight_norms(isac_ctx* ctx, const char* who, const isac_c64* W, int A, int B, std::vector<double>& norm);
int beam_planes_enqueue(isac_ctx* ctx, const isac::c64* d_Y, long long n_cells, const isac::c64* d_W, const double* d_norm, int B, double* d_Pb);
// ---------------------------------------------------------------- clean.hip: isac_fft2d_clean_targets (include/isac_clean.h) -- successive cancellation on a residual copy of the range rows of the last completed
// fft2D.  Reads ctx->tgt and ctx->ymid, writes ctx->clean / clean_det / clean_sel (and ctx->tgt_part through target_scan_snapshots) only; calls rdm_window_enqueue, cfar_detect_planes,
// target_cells_of_planes, tone_plan / refine_enqueue and target_scan_snapshots.
// For relax.hip and beam_clean.hip: the caller's sym_active [L] (NULL: every symbol) as the mask the kernels read and the number of active symbols
// (ISAC_ERR_INVALID_ARG: none)
namespace isac { struct SymbolMask { std::vector<unsigned char> act; int n_active = 0; }; }
int symbol_mask(isac_ctx* ctx, const char* who, const uint8_t* sym_active, int L, isac::SymbolMask* mask);
// For beam_clean.hip: what a cancellation loop carries across its passes, and steps 4-8 of isac_clean.h -- all of a pass that does not depend on how its cell was found.
// The entry point fills the first two lines; the loop owns n_iter's target and kept.
namespace isac {
struct CancelRecord { int wr, k, status, bin; double nu, power; };   // device, one copy back per pass: the picked cell [window row | k], refine_kernel's and the scan's results
static_assert(sizeof(CancelRecord) == 32, "the record and [nu | power] are fetched as one block of 32 bytes");
struct CancelLoop {
  const char* who; RefinePlan plan; c64* d_R /* [nr x L x A] */; CancelRecord* d_rec; c64* d_snap /* [A x max_iter] */; const unsigned char* d_act /* [L] */; int n_active, span_rows; double merge_tol;
  int32_t *n_iter, *row, *col, *status, *parent; double *nu, *vel, *power, *azi, *ele /* or NULL */;   // the caller's outputs
  int kept = 0;
};
}
// entry i = *n_iter at the 1-based cell (row, col): its tone (refine_kernel on d_R), direction, velocity and parent into the outputs, *n_iter = i + 1; then either *stop
// (status 1: nothing is subtracted) or clean_cancel_kernel enqueued on the window rows *span
int cancel_pass(isac_ctx* ctx, isac::CancelLoop& s, int row, int col, isac::RowSpan* span, bool* stop);
// behind the last pass: *n_kept, the first *n_iter snapshots and the residual rows (either may be NULL)
int cancel_finish(isac_ctx* ctx, const isac::CancelLoop& s, int32_t* n_kept, isac_c64* snapshots, isac_c64* residual_rows);
// ---------------------------------------------------------------- beam_clean.hip: isac_fft2d_beam_clean_targets (include/isac_beam_clean.h) -- successive cancellation with the detector on beam planes of a
// residual copy of the range rows of the last completed fft2D; planes, flags and the map over the beams stay on the device across the passes and are updated by row band.  Reads
// ctx->tgt and ctx->ymid, writes ctx->beam_clean (and ctx->tgt_part through target_scan_snapshots) only; calls rdm_window_enqueue, beam_weight_norms / beam_planes_enqueue,
// cfar_flag_planes, symbol_mask, tone_plan and cancel_pass / cancel_finish.
// ---------------------------------------------------------------- relax.hip: isac_fft2d_relax_targets (include/isac_relax.h) -- joint re-fit of Doppler tones on a residual copy of the range rows of the last
// completed fft2D.  Reads ctx->tgt and ctx->ymid, writes ctx->relax (and ctx->tgt_part through target_scan_snapshots) only; calls symbol_mask, tone_plan and target_scan_snapshots.
// ---------------------------------------------------------------- directions.hip: isac_resolve_directions (include/isac_directions.h) -- off-grid direction finding with several sources per array snapshot.
// Reads nothing of the context, writes ctx->directions only; calls and is called by no other unit (its steering spacing: upa_steer.hpp).
// ---------------------------------------------------------------- fft2d.hip: the host side of the fft2D pipeline -- submit, collect, submit_n / collect_n, the host-array call, the getters
// host half of fft2D.m:63-99 on per-antenna CUT-order lists (callers: isac_fft2d_collect, isac_fft2d_redetect)
int fft2d_estimates(isac_ctx* ctx, const isac_est_params* ep, const isac::CutWindow& win, int A, const int* ant_off, const std::vector<int>& cut, const std::vector<double>& pw, int num_dets_dev, std::vector<int32_t>& det_rc, isac_est_result* out);
// ---------------------------------------------------------------- cov.hip
int isac_covariance_on(isac_ctx* ctx, hipStream_t st, const isac_c64* d_grid, int64_t N, int32_t A, isac_c64* d_Ra);
int isac_covariance_lazy_on(isac_ctx* ctx, hipStream_t st, isac_c64* d_Ra);   // Ra of the context's native lazy echo grid
// The split route of that covariance (ISAC_LAZY_COV_SPLIT): what the head of the CPI hands to cov_noise_beam_kernel
struct LazySplitFront {
  const isac::c64* d_tx; long long T; int A, Q;
  const isac::c64* steer_host;   // [A x Q] compacted LoS columns for the argument block, or nullptr: they are in ctx->steer
  isac::BeamWindow bw;
  int K, L_whole, L_out; unsigned long long seed;
};
bool isac_lazy_split_ok(long long T, int K, int L_whole);
int isac_cov_noise_beam_on(isac_ctx* ctx, hipStream_t st, const LazySplitFront& f);   // noise partials -> ctx->cov_noise, beam-sums -> ctx->beam (inside f.bw's ranges), ctx->steer
// ctx->cov_xc: cross partials [L_whole][A][Q] (echo_range_xc_kernel) | D's Gram matrix per symbol [L_whole][Q][Q] | M / N [A x A]
inline size_t lazy_xc_elems(int L_whole, int A, int Q) { return (size_t)L_whole * A * Q; }
inline size_t lazy_xc_total(int L_whole, int A, int Q) { return lazy_xc_elems(L_whole, A, Q) + (size_t)L_whole * Q * Q + (size_t)A * A; }
// ---------------------------------------------------------------- multistatic.hip: the coefficient vectors of a multi-static echo (include/isac_multistatic.h), for echo.hip's two entry points
// The arguments of those calls, checked by the caller (limits, indices, shifts >= 0, the named sources' waveforms and element counts); every array is a host array.
struct PathCoefJob {
  const isac::c64* const* d_tx; const int32_t* n_ants_src;   // [S] device pointers, element counts
  long long T; double fc, fs; int n_ants, n_paths;
  const int32_t* path_source; const int64_t* path_shift; const double* path_doppler_hz; const double* path_gain;
  const isac_c64* path_tx_steering; const isac_c64* path_rx_steering;
};
int isac_path_coefs_on(isac_ctx* ctx, hipStream_t st, const PathCoefJob& j);   // coef [P x T] -> ctx->coef, phase_rx [T] -> ctx->phase_rx, rx steering [A x P] and its transpose -> ctx->steer
// The fractional delays of include/isac_subsample.h on the demodulated coefficient grids D [n_sc x L_whole x P] in ctx->dgrid: D_p <- D_p exp(-2 pi j (frac(fc delta_p / fs) +
// m_k delta_p / Nfft)), one element-wise launch on st; a path with delta_p == 0 keeps its bits.  frac [P]: host, every value in [0, 1), at least one not zero (checked by the caller).
struct PathFrac { const double* frac; double fc, fs; };
int isac_path_frac_ramp_on(isac_ctx* ctx, hipStream_t st, const PathFrac& f, int n_sc, int nfft, int L_whole, int n_paths);
// ---------------------------------------------------------------- range_refine.hip: isac_range_refine_dev (include/isac_subsample.h) -- off-grid range of listed targets from the two grids of a CPI.  Reads
// nothing of the context but the cached Kaiser window (isac_get_windows), writes ctx->range_refine only; calls and is called by no other unit.
// ---------------------------------------------------------------- localize.hip: isac_position_map_dev, isac_localize_dev (include/isac_localize.h) -- per-link lists fused into positions.  Reads nothing of the
// context, writes ctx->localize only; calls and is called by no other unit.
// ---------------------------------------------------------------- track.hip: isac_track_state_bytes, isac_track_reset_dev, isac_track_step_dev, isac_track_get_dev (include/isac_track.h) -- Kalman track banks
// across CPIs.  Reads nothing of the context, writes ctx->track (and the caller's state block) only; calls and is called by no other unit.
// ---------------------------------------------------------------- cancel_paths.hip: isac_cancel_paths_dev (include/isac_cancel_paths.h) -- known reference signals projected out of a received waveform.  Calls
// isac_path_coefs_on (unit gains, one receive element: the reference columns R [M x T] in ctx->coef; ctx->steer and ctx->phase_rx are rewritten with them) and is called by no
// other unit; its own scratch is ctx->cancel_paths.
// ---------------------------------------------------------------- eigh.hip (the device code it shares with music.hip: eigh_dev.hpp)
// device eig: H [A x A] (device) -> ctx->eig_w [A], ctx->eig_v [A x A] (unsorted); live_replay: see the definition
int isac_eigh_dev(isac_ctx* ctx, const isac::c64* d_H, int A, hipStream_t st, bool live_replay = true);
int isac_eigh_replay_recover(isac_ctx* ctx, int n, hipStream_t st);
int isac_eigh_ql_dev(isac_ctx* ctx, int n, hipStream_t st, const int* ctl, bool allow_live = true);   // the QL pipeline on the tridiagonal form in ctx->eig_scratch; ctl: see the definition
int isac_music_tridiag_bisect_dev(isac_ctx* ctx, const isac::c64* d_H, int A, hipStream_t st);           // first half of MUSIC's signal-subspace route (before numDets)
// ---------------------------------------------------------------- music.hip
// MUSIC's signal-subspace eigensolver: usable for this order?  second half (after numDets), its control block
bool isac_music_subspace_ok(isac_ctx* ctx, int A);
int isac_music_subspace_dev(isac_ctx* ctx, int A, const int* d_num_dets, int num_dets_host, hipStream_t st);
const int* isac_music_ctl(isac_ctx* ctx);
int isac_music_scan_dev(isac_ctx* ctx, int A, const int* d_num_dets, int num_dets_host, const double* d_sind, int n_steps, double d_ratio, double* d_spec, hipStream_t st, int mode = 0, const int* ctl = nullptr);
// music2D stages (host side: doa.hip)
int isac_music2d_plane(isac_ctx* ctx, const isac::c64* d_rx, const isac::c64* d_tx, long long n, isac::c64* d_h);
int isac_music2d_signal_vectors(isac_ctx* ctx, const isac::c64* d_h, int K, int Ls, const int* d_top, int Lsig, isac::c64* d_U);
int isac_music2d_scan(isac_ctx* ctx, const isac::c64* d_U, int N, int ldU, const int* d_cols, int Lsig, int conj_u, double coef, double den, double x0, double dx, int n_steps, double* d_p);
// ---------------------------------------------------------------- doa2d.hip: UPA DoA -- the 2-D scan, the column normalisation + peak candidates, the host sort of find2DPeaks (callers: doa.hip)
int isac_doa2d_peak_cap(int rows, int cols);
int isac_doa2d_cand_doubles(int cap);
int isac_doa2d_scan_dev(isac_ctx* ctx, int mode, int nV, int nH, int eS, int aS, const double* d_tab, const int* d_num_dets, int num_dets_host, const int* ctl, hipStream_t st);
int isac_doa2d_norm_peaks_dev(isac_ctx* ctx, bool normalise, const double* d_db, int rows, int cols, double* d_cand, int cap, hipStream_t st);
int isac_doa2d_select(isac_ctx* ctx, const double* cand, int count, int cap, int rows, int L, std::vector<int>& ele, std::vector<int>& azi);
// ---------------------------------------------------------------- doa.hip: the host side of direction finding, one back end for the fft2D pipeline and the stand-alone calls
int doa_plan(isac_ctx* ctx, const isac_est_params* ep, int A, int mode, isac::DoaPlan* pl);   // route, scan tables, every buffer of the tail; enqueues nothing
constexpr const char* kUpaRefused = "UPA DoA: music.m:69 calls tools.find2DPeaks, which the reference does not define";   // ISAC_ERR_UNSUPPORTED where plan.refused()
int doa_eig_first_half(isac_ctx* ctx, const isac::DoaPlan& pl, const isac::c64* d_H, hipStream_t st, bool live_replay);
int doa_enqueue(isac_ctx* ctx, const isac::DoaPlan& pl, const int* d_num_dets, int num_dets_host, hipStream_t st);   // subspace -> scan (-> norm + peak candidates)
int doa_readout(isac_ctx* ctx, const isac::DoaPlan& pl, const isac_est_params* ep, const double* host, int n_first, int L, const char* none_prefix, std::vector<double>& ele, std::vector<double>& azi);
void doa_store(const std::vector<double>& ele, const std::vector<double>& azi, int n, double* ele_est, double* azi_est);   // the first n, NaN elevations for a ULA
int isac_doa2d_grid(isac_ctx* ctx, const isac_est_params* ep, int A, const double** d_tab, int* e_steps, int* a_steps);   // UPA dims checked against A, then the cached [sind(ele) | cosd(azi) | sind(azi)] table (caller: targets.hip)
// ---------------------------------------------------------------- cdl_os.hip: the CDL apply in the frequency domain (overlap-save, 4096-point windows) for long waveforms
bool cdl_os_ok(long long T, int Nt, int Nr, int n_paths, int n_taps, int max_shift);      // downlink: into two receive elements
bool cdl_os_ul_ok(long long T, int Nt, int Nr, int n_paths, int n_taps, int max_shift);   // uplink: one or two transmit elements into many receive elements
int cdl_os_apply(isac_ctx* ctx, const isac_cdl_job* jobs, int n_jobs, long long T, int Nt, int Nr, int n_paths, const double* taps, int n_taps, const int32_t* shift, int max_shift, double out_scale);
// ---------------------------------------------------------------- rxfe.hip: the tail of applyChannelModel (path loss, Rx gain, thermal noise), one launch for a batch
constexpr uint32_t kRxFrontEndStream = 3u;   // Philox stream word of its time-domain AWGN (0: the echo's time-domain noise, 1: isac_synth_qpsk_grid_dev, 2: kSpectralStream)
constexpr uint32_t kCfarMcStream = 4u;       // ... 4: the noise cells of isac_cfar_monte_carlo (cfar.hip; include/isac_cfar_mc.h)
int isac_rx_frontend_jobs(isac_ctx* ctx, const isac_rx_frontend_job* jobs, int n_jobs, long long T, int Nr, int noise_mode);

// The status record the device eigensolver leaves behind the eigenvalues (ctx->eig_w [A] | isac::EighInfo, eigh_layout.hpp), and the one place the two outputs are sized
inline isac::EighInfo* eig_info(isac_ctx* ctx, int A) { return reinterpret_cast<isac::EighInfo*>((char*)ctx->eig_w.p + sizeof(double) * (size_t)A); }
inline int ensure_eig_out(isac_ctx* ctx, int A) {   // ctx->eig_w [A] + the record, ctx->eig_v [A x A]
  ISAC_TRY(isac::ensure(ctx, ctx->eig_w, sizeof(double) * (size_t)A + sizeof(isac::EighInfo)));
  return isac::ensure(ctx, ctx->eig_v, sizeof(isac::c64) * (size_t)A * A);
}
namespace isac {
hipEvent_t timeline_base(hipStream_t st);   // fft2d.hip
inline void timeline_mark(isac_ctx* ctx, int i, hipStream_t st) {
  static const bool on = std::getenv("ISAC_TIMELINE") != nullptr;   // diagnostic: per-stage event timeline
  if (!on) return;
  if (!ctx->tl_on) {
    for (auto& e : ctx->tl) (void)hipEventCreate(&e);
    ctx->tl_on = true;
    (void)timeline_base(st);
  }
  (void)hipEventRecord(ctx->tl[i], st);
}

struct MusicCtl { enum { kRoute = 0, kLsub = 1 }; };     // MUSIC's control block (isac_music_ctl): ctl[kRoute]: 1 = subspace vectors delivered (kLsub of them; >= n: empty noise space)
}  // namespace isac
