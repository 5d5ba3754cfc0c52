// Direction finding on the host (gfx950 only): the one DoA back end behind the fft2D pipeline (fft2d.hip) and the stand-alone calls, the stand-alone
// eigensolver calls, find2DPeaks and music2D.  No kernel lives here: the eigensolver is eigh.hip, the scans are music.hip (ULA) and doa2d.hip (UPA).
#include <algorithm>
#include <numeric>

#include "isac_internal.hpp"

using namespace isac;

namespace {

int eig_status(isac_ctx* ctx, int A, bool ql_ran = true /* false: the signal-subspace kernel delivered, the QL pipeline returned at once */) {
  int sweeps = 0;
  ISAC_TRY(copy_d2h(ctx, &sweeps, &eig_info(ctx, A)->status, sizeof(int)));
  static const bool force = std::getenv("ISAC_EIG_FORCE_REPLAY_TIMEOUT") != nullptr;   // test hook: take the recovery path on every call ...
  if (force && ql_ran && sweeps >= 0 && A > 16 && ctx->eig_scratch.p) {
    ISAC_HIP(hipMemset(ctx->eig_v.p, 0xFF, sizeof(c64) * (size_t)A * A));               // ... with the eigenvectors destroyed first
    sweeps = kEighReplayTimeout;
  }
  if (sweeps == kEighReplayTimeout) {                                // live replay blocks gave up waiting: Z and the rotations are intact, replay them offline
    ISAC_TRY(isac_eigh_replay_recover(ctx, A, ctx->stream));
    ISAC_HIP(hipStreamSynchronize(ctx->stream));
    ISAC_TRY(copy_d2h(ctx, &sweeps, &eig_info(ctx, A)->status, sizeof(int)));
  }
  if (sweeps < 0) return isac::fail(ctx, ISAC_ERR_HIP, sweeps == kEighRotStorage ? "eigensolver: QL recurrence exceeded its rotation storage (no convergence)"
                                                     : sweeps == kEighNotFinite ? "eigensolver: the signal-subspace vectors are not finite (NaN / Inf in the covariance)"
                                                     : sweeps == kEighTridiagTimeout ? "eigensolver: the distributed tridiagonalisation saw no progress for 2 s (its workgroups were not resident together)"
                                                                     : "eigensolver: a replay block timed out waiting for the recurrence");
  return ISAC_OK;
}

// ---- host math mirrors of the MATLAB helpers the reference calls (product code, not the oracle)
double sind_deg(double x) {  // degree-domain reduction: exact at multiples of 90, sind(180-p) == sind(p) bitwise
  x = std::fmod(x, 360.0);
  if (x > 180.0) x -= 360.0;
  if (x < -180.0) x += 360.0;
  if (x > 90.0) x = 180.0 - x;
  if (x < -90.0) x = -180.0 - x;
  const double ax = std::fabs(x);
  const double k = M_PI / 180.0;
  if (ax <= 45.0) return std::sin(x * k);
  const double c = std::cos((90.0 - ax) * k);
  return x < 0 ? -c : c;
}

double cosd_deg(double x) {  // cosd via sind(90 - |x|) (oracle/matlab_compat.py): even, exact zeros at +-90, cosd(p - 180) == -cosd(p) bitwise
  return sind_deg(90.0 - std::fmod(std::fabs(x), 360.0));
}

// findpeaks(y,'NPeaks',L,'SortStr','descend'): strict maxima, first sample of plateaus, no end points,
// stable descending sort (music.m:102).  Returns 0-based locations.
std::vector<int> findpeaks_desc(const std::vector<double>& y, int npeaks) {
  std::vector<int> idx;
  const int n = (int)y.size();
  for (int i = 0; i < n; ++i)
    if (i == 0 || y[(size_t)i] != y[(size_t)i - 1]) idx.push_back(i);
  std::vector<int> locs;
  for (size_t k = 1; k + 1 < idx.size(); ++k) {
    double a = y[(size_t)idx[k - 1]], b = y[(size_t)idx[k]], c = y[(size_t)idx[k + 1]];
    if (b > a && b > c) locs.push_back(idx[k]);
  }
  std::stable_sort(locs.begin(), locs.end(), [&](int p, int q) { return y[(size_t)p] > y[(size_t)q]; });
  if ((int)locs.size() > npeaks) locs.resize((size_t)npeaks);
  return locs;
}

int determine_num_targets(const std::vector<double>& v_ascending) {  // music.m:109-125 (on eig()'s ascending order)
  const int n = (int)v_ascending.size() - 1;
  if (n < 1) return 1;
  std::vector<double> delta((size_t)n);
  for (int i = 0; i < n; ++i) delta[(size_t)i] = -(v_ascending[(size_t)i + 1] - v_ascending[(size_t)i]);
  const int start = (int)std::ceil((n + 1) / 2.0) - 1;
  double sum = 0.0;
  for (int i = start; i < n; ++i) sum += delta[(size_t)i];
  const double half_mean = sum / (double)(n - start);
  int best = 0;
  double bv = delta[0] - 2.0 * half_mean;
  for (int i = 1; i < n; ++i) {
    double v = delta[(size_t)i] - 2.0 * half_mean;
    if (v > bv) { bv = v; best = i; }
  }
  return best + 1;
}

int scan_steps(const isac_est_params* ep) {
  return (int)std::floor((ep->azimuth_scan_scale + 1.0) / ep->azimuth_scan_granularity);   // music.m:79
}

int get_sind_table(isac_ctx* ctx, const isac_est_params* ep, const double** out, int* n_steps) {
  const int n = scan_steps(ep);
  if (n <= 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "empty azimuth scan");
  *n_steps = n;
  return cached_table(ctx, {kSind, {std::llround(ep->azimuth_scan_scale * 1e6), std::llround(ep->azimuth_scan_granularity * 1e6)}}, out, [&](std::vector<double>& s) {
    s.resize((size_t)n);
    for (int a = 0; a < n; ++a) s[(size_t)a] = sind_deg(a * ep->azimuth_scan_granularity - ep->azimuth_scan_scale / 2.0);   // music.m:88
  });
}

// UPA scan grid (music.m:36-53): eSteps x aSteps points, row e at elevation (e-1) eGran - eMax/2, column a at azimuth (a-1) aGran - aMax/2.
// Device table [sind(ele) eSteps | cosd(azi) aSteps | sind(azi) aSteps], made on the host once per grid.
int get_doa2d_tables(isac_ctx* ctx, const isac_est_params* ep, const double** out, int* e_steps, int* a_steps) {
  const double ag = ep->azimuth_scan_granularity, am = ep->azimuth_scan_scale, eg = ep->elevation_scan_granularity, em = ep->elevation_scan_scale;
  if (!(ag > 0.0) || !(eg > 0.0) || !std::isfinite(am) || !std::isfinite(em)) return fail(ctx, ISAC_ERR_INVALID_ARG, "UPA DoA: scan scales / granularities");
  const double ne = std::floor((em + 1.0) / eg), na = std::floor((am + 1.0) / ag);                     // music.m:42-43
  if (!(ne >= 1.0) || !(na >= 1.0) || ne * na > (double)(1 << 26)) return fail(ctx, ISAC_ERR_INVALID_ARG, "UPA DoA: empty or oversized scan grid");
  const int n_e = (int)ne, n_a = (int)na;
  *e_steps = n_e;
  *a_steps = n_a;
  return cached_table(ctx, {kDoa2d, {std::llround(am * 1e6), std::llround(ag * 1e6), std::llround(em * 1e6), std::llround(eg * 1e6)}}, out, [&](std::vector<double>& t) {
    t.resize((size_t)n_e + 2 * (size_t)n_a);
    for (int e = 0; e < n_e; ++e) t[(size_t)e] = sind_deg(e * eg - em / 2.0);                         // music.m:47,44
    for (int a = 0; a < n_a; ++a) {
      const double ph = a * ag - am / 2.0;                                                              // music.m:48
      t[(size_t)n_e + a] = cosd_deg(ph);
      t[(size_t)n_e + n_a + a] = sind_deg(ph);
    }
  });
}

int check_upa_dims(isac_ctx* ctx, const isac_est_params* ep, int A) {   // radarParams.m:90,99 reshape to nTxAnts
  if (ep->n_ants_x <= 0 || ep->n_ants_y <= 0 || (long long)ep->n_ants_x * ep->n_ants_y != A)
    return fail(ctx, ISAC_ERR_INVALID_ARG, "UPA DoA: n_ants_x * n_ants_y must equal the number of antennas");
  if (A > 256) return fail(ctx, ISAC_ERR_UNSUPPORTED, "UPA DoA: the 2-D scan supports up to 256 elements");
  return ISAC_OK;
}

void to_db(std::vector<double>& v) {   // 20 log10(|p| / max |p|)   music.m:94-96
  double mx = 0.0;
  for (double x : v) mx = std::max(mx, std::fabs(x));
  for (double& x : v) x = 20.0 * std::log10(std::fabs(x) / mx);
}
// 0-based scan bins -> degrees   music.m:103 (ULA), :70-71 (UPA, from find2DPeaks' 1-based bins)
double azi_deg(const isac_est_params* ep, int bin) { return bin * ep->azimuth_scan_granularity - ep->azimuth_scan_scale / 2.0; }
double ele_deg(const isac_est_params* ep, int bin) { return bin * ep->elevation_scan_granularity - ep->elevation_scan_scale / 2.0; }

// music.m:94-104 on a raw spectrum: to dB in place, then the L largest peaks in degrees
int ula_peaks(isac_ctx* ctx, const isac_est_params* ep, std::vector<double>& spec, int L, const std::string& none_msg, std::vector<double>& azi) {
  to_db(spec);
  if (L <= 0) return fail(ctx, ISAC_ERR_NO_DETECTION, none_msg);
  for (int loc : findpeaks_desc(spec, L)) azi.push_back(azi_deg(ep, loc));   // :102-103
  return ISAC_OK;
}

// Host half of find2DPeaks on the candidate list [counter | candidates] at d_cand: count -> bound -> the list -> the L largest as 1-based bins.  `first`: the
// head of the list with room for n_first candidates when the caller holds it on the host already (NULL: nothing yet); only what lies beyond it is fetched.
int fetch_select(isac_ctx* ctx, const double* first, int n_first, const double* d_cand, int cap, int rows, int L, const char* none_prefix,
                 std::vector<int>& ele, std::vector<int>& azi) {
  unsigned count = first ? *(const unsigned*)first : 0;
  if (!first) ISAC_TRY(copy_d2h(ctx, &count, d_cand, sizeof(count)));
  if ((int)count > cap) return fail(ctx, ISAC_ERR_HIP, "find2DPeaks: candidate count beyond the 2 x 2 bound (internal error)");
  if (L <= 0) return fail(ctx, ISAC_ERR_NO_DETECTION, std::string(none_prefix) + "find2DPeaks needs a positive number of peaks (music.m:69)");
  std::vector<double> full;
  if (!first || (int)count > n_first) {
    full.resize((size_t)isac_doa2d_cand_doubles((int)count));
    ISAC_TRY(copy_d2h(ctx, full.data(), d_cand, sizeof(double) * full.size()));
    first = full.data();
  }
  return isac_doa2d_select(ctx, first, (int)count, cap, rows, L, ele, azi);
}

// ---- eigenvalues / eigenpairs on the host
int num_targets_of_eig(isac_ctx* ctx, int A, int* L) {   // determineNumTargets on the eigenvalues in ctx->eig_w, put into eig()'s ascending order first
  std::vector<double> wv((size_t)A);
  ISAC_TRY(copy_d2h(ctx, wv.data(), ctx->eig_w.p, sizeof(double) * (size_t)A));
  ISAC_HIP(hipStreamSynchronize(ctx->stream));
  std::sort(wv.begin(), wv.end());
  *L = determine_num_targets(wv);
  return ISAC_OK;
}

// The eigenpairs of ctx->eig_w / eig_v on the host (vv == NULL: the eigenvalues only) and the (stable) order that sorts the eigenvalues
int sorted_eigenpairs(isac_ctx* ctx, int A, bool descending, std::vector<double>& wv, std::vector<c64>* vv, std::vector<int>& order) {
  wv.resize((size_t)A); if (vv) vv->resize((size_t)A * A);
  ISAC_TRY(copy_d2h(ctx, wv.data(), ctx->eig_w.p, sizeof(double) * (size_t)A));           // (the context's streams are
  if (vv) ISAC_TRY(copy_d2h(ctx, vv->data(), ctx->eig_v.p, sizeof(c64) * (size_t)A * A));  //  non-blocking: stay on them)
  ISAC_HIP(hipStreamSynchronize(ctx->stream));
  ISAC_TRY(eig_status(ctx, A));
  order.resize((size_t)A);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int p, int q) { return descending ? wv[(size_t)p] > wv[(size_t)q] : wv[(size_t)p] < wv[(size_t)q]; });
  return ISAC_OK;
}

int eig_debug_print(isac_ctx* ctx, int A, int n_top /* < 0: isac_eigh */) {   // ISAC_DEBUG diagnostic: eigensolver phase counters on stderr
  if (!std::getenv("ISAC_DEBUG")) return ISAC_OK;
  EighInfo inf{};
  ISAC_TRY(copy_d2h(ctx, &inf, eig_info(ctx, A), sizeof(inf)));
  if (n_top >= 0)
    std::fprintf(stderr, "[isac] eigh_top A=%d n_top=%d phases(x64 clk): tridiag=%d (n <= 64: reflector=%d matvec=%d matvec+update=%d) | subspace: set-up=%d solves=%d "
                 "gram-schmidt=%d back-transform=%d\n", A, n_top, inf.cyc_a, inf.tri_a, inf.tri_b, inf.tri_c, inf.sub_setup, inf.sub_solve, inf.sub_mgs, inf.sub_back);
  else {
    if (A > 64 && A <= 256)
      std::fprintf(stderr, "[isac] eigh A=%d distributed tridiagonalisation, phases(x64 clk): column + p published=%d exchange wait=%d vector work=%d rank-2 update=%d\n", A,
                   inf.tri_a, inf.tri_b, inf.tri_c, inf.tri_d);
    if (inf.rotations < 0)
      std::fprintf(stderr, "[isac] eigh A=%d Jacobi sweeps=%d phases(x64 clk): rotation parameters=%d two-sided updates=%d\n", A, inf.status, inf.cyc_a, inf.cyc_b);
    else
      std::fprintf(stderr, "[isac] eigh A=%d QL sweeps=%d rotations=%d phases(x64 clk): tridiag=%d formQ=%d ql-recurrence=%d replay=%d\n", A, inf.status,
                   inf.rotations, inf.cyc_a, inf.cyc_b, inf.cyc_ql, inf.cyc_replay);
  }
  return ISAC_OK;
}

}  // namespace

// The UPA scan grid for a caller outside the DoA back end (targets.hip): nV x nH against A and the 256-element limit of the 2-D scans, then the cached table
int isac_doa2d_grid(isac_ctx* ctx, const isac_est_params* ep, int A, const double** d_tab, int* e_steps, int* a_steps) {
  ISAC_TRY(check_upa_dims(ctx, ep, A));
  return get_doa2d_tables(ctx, ep, d_tab, e_steps, a_steps);
}

// ------------------------------------------------------------------ the DoA back end: plan -> first half of the eigen stage -> scan -> read-out
// Everything both callers settle before anything is enqueued: which route, the scan tables, every buffer of the tail.
int doa_plan(isac_ctx* ctx, const isac_est_params* ep, int A, int mode, DoaPlan* pl) {
  *pl = DoaPlan{};
  pl->A = A; pl->mode = mode;
  pl->upa = ep->array_is_upa != 0;
  pl->upa2d = pl->upa && ctx->upa_doa != 0;                                                    // ISAC_OPT_UPA_DOA
  pl->sub = mode == 0 && !pl->refused() && isac_music_subspace_ok(ctx, A);
  if (!pl->upa) {
    ISAC_TRY(get_sind_table(ctx, ep, &pl->d_sind, &pl->n_steps));
    ISAC_TRY(ensure(ctx, ctx->spec, sizeof(double) * (size_t)pl->n_steps));
  }
  if (pl->upa2d) {
    ISAC_TRY(check_upa_dims(ctx, ep, A));
    ISAC_TRY(get_doa2d_tables(ctx, ep, &pl->d_tab2d, &pl->e_steps, &pl->a_steps));
    pl->cap2d = isac_doa2d_peak_cap(pl->e_steps, pl->a_steps);
    pl->n_ants_x = ep->n_ants_x; pl->n_ants_y = ep->n_ants_y;
    const size_t n_pts = (size_t)pl->e_steps * pl->a_steps;
    ISAC_TRY(ensure(ctx, ctx->doa2d_p, sizeof(double) * n_pts));                               // (these two are what isac_doa2d_scan_dev would size at its launch)
    ISAC_TRY(ensure(ctx, ctx->doa2d_w, sizeof(double) * (size_t)A));
    ISAC_TRY(ensure(ctx, ctx->doa2d_db, sizeof(double) * n_pts));
    ISAC_TRY(ensure(ctx, ctx->doa2d_cand, sizeof(double) * (size_t)isac_doa2d_cand_doubles(pl->cap2d)));
  }
  return ISAC_OK;
}

// music.m:19, the part that does not depend on numDets: reflectors + eigenvalues of the signal-subspace route, or the whole eigendecomposition
int doa_eig_first_half(isac_ctx* ctx, const DoaPlan& pl, const c64* d_H, hipStream_t st, bool live_replay) {
  return pl.sub ? isac_music_tridiag_bisect_dev(ctx, d_H, pl.A, st) : isac_eigh_dev(ctx, d_H, pl.A, st, live_replay);
}

// The numDets signal vectors (or the QL fallback), then the ULA scan (music.m:82-91), or the 2-D scan + the device half of find2DPeaks (music.m:31-63 /
// digitalBF.m:13-53 / mvdrBF.m:13-53).  numDets: the device word d_num_dets, or num_dets_host when that is NULL.
int doa_enqueue(isac_ctx* ctx, const DoaPlan& pl, const int* d_num_dets, int num_dets_host, hipStream_t st) {
  if (pl.refused()) return ISAC_OK;
  if (pl.sub) ISAC_TRY(isac_music_subspace_dev(ctx, pl.A, d_num_dets, num_dets_host, st));
  const int* ctl = pl.sub ? isac_music_ctl(ctx) : nullptr;
  if (!pl.upa) return isac_music_scan_dev(ctx, pl.A, d_num_dets, num_dets_host, pl.d_sind, pl.n_steps, 0.5, (double*)ctx->spec.p, st, pl.mode, ctl);
  ISAC_TRY(isac_doa2d_scan_dev(ctx, pl.mode, pl.n_ants_x, pl.n_ants_y, pl.e_steps, pl.a_steps, pl.d_tab2d, d_num_dets, num_dets_host, ctl, st));
  return isac_doa2d_norm_peaks_dev(ctx, true, (const double*)ctx->doa2d_db.p, pl.e_steps, pl.a_steps, (double*)ctx->doa2d_cand.p, pl.cap2d, st);
}

// From what the scan left to the estimates in degrees (ele stays empty for a ULA).  `host`: what the caller holds on the host already -- the raw ULA spectrum
// [n_steps], or the first n_first peak candidates of the UPA; NULL: nothing yet, fetched here.  Fills last.spectrum_db (ULA) / records the dims of the dB map
// (UPA) before it reports L <= 0; none_prefix goes in front of that report's text.
int doa_readout(isac_ctx* ctx, const DoaPlan& pl, const isac_est_params* ep, const double* host, int n_first, int L, const char* none_prefix,
                std::vector<double>& ele, std::vector<double>& azi) {
  if (!pl.upa) {
    std::vector<double>& db = ctx->last.spectrum_db;
    if (host) db.assign(host, host + pl.n_steps);
    else { db.resize((size_t)pl.n_steps); ISAC_TRY(copy_d2h(ctx, db.data(), ctx->spec.p, sizeof(double) * db.size())); }
    return ula_peaks(ctx, ep, db, L, std::string(none_prefix) + "findpeaks 'NPeaks' must be a positive integer (music.m:102)", azi);
  }
  ctx->doa2d_rows = pl.e_steps; ctx->doa2d_cols = pl.a_steps;
  std::vector<int> e, a;
  ISAC_TRY(fetch_select(ctx, host, n_first, (const double*)ctx->doa2d_cand.p, pl.cap2d, pl.e_steps, L, none_prefix, e, a));
  for (size_t i = 0; i < a.size(); ++i) { ele.push_back(ele_deg(ep, e[i] - 1)); azi.push_back(azi_deg(ep, a[i] - 1)); }
  return ISAC_OK;
}

void doa_store(const std::vector<double>& ele, const std::vector<double>& azi, int n, double* ele_est, double* azi_est) {
  for (int i = 0; i < n; ++i) {
    if (azi_est) azi_est[i] = azi[(size_t)i];
    if (ele_est) ele_est[i] = ele.empty() ? NAN : ele[(size_t)i];   // ULA: music.m:104
  }
}

// ------------------------------------------------------------------ stand-alone eig
extern "C" int isac_eigh(isac_ctx* ctx, const isac_c64* H, int32_t A, double* w, isac_c64* V) {
  ISAC_ENTER(ctx);
  if (!H || !w || A <= 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "bad arguments");
  ISAC_TRY(upload(ctx, ctx->stage_c, H, sizeof(c64) * (size_t)A * A));
  ISAC_TRY(isac_eigh_dev(ctx, (const c64*)ctx->stage_c.p, A, nullptr));
  std::vector<double> wv; std::vector<c64> vv; std::vector<int> order;
  ISAC_TRY(sorted_eigenpairs(ctx, A, false, wv, &vv, order));
  ISAC_TRY(eig_debug_print(ctx, A, -1));
  for (int i = 0; i < A; ++i) {
    w[i] = wv[(size_t)order[(size_t)i]];
    if (V) std::memcpy(V + (size_t)A * i, vv.data() + (size_t)A * order[(size_t)i], sizeof(c64) * (size_t)A);
  }
  return ISAC_OK;
}

// eigenvalues (all, ascending) + the eigenvectors of the n_top largest, through MUSIC's signal-subspace route
extern "C" int isac_eigh_top(isac_ctx* ctx, const isac_c64* H, int32_t A, int32_t n_top, double* w, isac_c64* U) {
  ISAC_ENTER(ctx);
  if (!H || !w || A <= 0 || n_top < 0 || n_top > A || (n_top > 0 && !U)) return fail(ctx, ISAC_ERR_INVALID_ARG, "bad arguments");
  if (A < 3 || A > 256) return fail(ctx, ISAC_ERR_UNSUPPORTED, "isac_eigh_top: orders 3..256 (use isac_eigh)");
  ISAC_TRY(upload(ctx, ctx->stage_c, H, sizeof(c64) * (size_t)A * A));
  ISAC_TRY(isac_music_tridiag_bisect_dev(ctx, (const c64*)ctx->stage_c.p, A, nullptr));
  ISAC_TRY(copy_d2h(ctx, w, ctx->eig_w.p, sizeof(double) * (size_t)A));
  ISAC_HIP(hipStreamSynchronize(ctx->stream));                      // (the fallback below overwrites eig_w with unsorted values)
  if (n_top == 0) return ISAC_OK;
  ISAC_TRY(isac_music_subspace_dev(ctx, A, nullptr, n_top, nullptr));
  int ctl[2] = {0, 0};
  ISAC_TRY(copy_d2h(ctx, ctl, isac_music_ctl(ctx), sizeof(ctl)));
  ISAC_HIP(hipStreamSynchronize(ctx->stream));
  ISAC_TRY(eig_status(ctx, A, ctl[0] != 1));
  ISAC_TRY(eig_debug_print(ctx, A, n_top));
  if (ctl[0] == 1 && n_top < A) {                                   // the subspace kernel delivered the vectors, descending eigenvalue order
    ISAC_TRY(copy_d2h(ctx, U, ctx->eig_v.p, sizeof(c64) * (size_t)A * n_top));
    ISAC_HIP(hipStreamSynchronize(ctx->stream));
    return ISAC_OK;
  }
  // n_top beyond the subspace kernel's capacity (or the whole basis): the QL pipeline ran; pick the columns of the n_top largest
  if (n_top == A) ISAC_TRY(isac_eigh_dev(ctx, (const c64*)ctx->stage_c.p, A, nullptr));
  std::vector<double> wv; std::vector<c64> vv; std::vector<int> order;
  ISAC_TRY(sorted_eigenpairs(ctx, A, true, wv, &vv, order));
  for (int i = 0; i < n_top; ++i) std::memcpy(U + (size_t)A * i, vv.data() + (size_t)A * order[(size_t)i], sizeof(c64) * (size_t)A);
  return ISAC_OK;
}

// ------------------------------------------------------------------ stand-alone MUSIC / digitalBF / mvdrBF
static int doa_scan(isac_ctx* ctx, int mode, int32_t num_dets, const isac_est_params* ep, const isac_c64* Ra, int32_t A,
                    int32_t* L_out, double* azi_est, double* ele_est, int32_t cap, int32_t* n_est) {
  ISAC_ENTER(ctx);
  if (!ep || !Ra || A <= 0 || !n_est) return fail(ctx, ISAC_ERR_INVALID_ARG, "bad arguments");
  *n_est = 0;
  ISAC_TRY(upload(ctx, ctx->stage_c, Ra, sizeof(c64) * (size_t)A * A));
  DoaPlan pl;
  ISAC_TRY(doa_plan(ctx, ep, A, mode, &pl));
  ISAC_TRY(doa_eig_first_half(ctx, pl, (const c64*)ctx->stage_c.p, nullptr, true));              // music.m:19 (a refused UPA too: its eigenvalues give L)
  int L = num_dets;
  if (num_dets < 0) ISAC_TRY(num_targets_of_eig(ctx, A, &L));                                      // music.m:21-22
  if (L_out) *L_out = L;
  if (pl.refused()) return fail(ctx, ISAC_ERR_UNSUPPORTED, kUpaRefused);
  ISAC_TRY(doa_enqueue(ctx, pl, nullptr, L, nullptr));
  ISAC_HIP(hipStreamSynchronize(ctx->stream));
  ISAC_TRY(eig_status(ctx, A));
  std::vector<double> ele, azi;
  ISAC_TRY(doa_readout(ctx, pl, ep, nullptr, 0, L, "", ele, azi));                                 // (fetches the spectrum / the peak candidates)
  if ((int)azi.size() > cap) return fail(ctx, ISAC_ERR_CAPACITY, "more peaks than capacity");
  *n_est = (int)azi.size();
  doa_store(ele, azi, *n_est, ele_est, azi_est);
  return ISAC_OK;
}

extern "C" int isac_music_doa(isac_ctx* ctx, int32_t num_dets, const isac_est_params* ep, const isac_c64* Ra, int32_t A,
                              int32_t* L_out, double* azi_est, double* ele_est, int32_t cap, int32_t* n_est) {
  return doa_scan(ctx, 0, num_dets, ep, Ra, A, L_out, azi_est, ele_est, cap, n_est);
}
extern "C" int isac_beamscan_doa(isac_ctx* ctx, int32_t method, int32_t num_dets, const isac_est_params* ep, const isac_c64* Ra,
                                 int32_t A, double* azi_est, double* ele_est, int32_t cap, int32_t* n_est) {
  if (method != 1 && method != 2) return fail(ctx, ISAC_ERR_INVALID_ARG, "method: 1 = digitalBF, 2 = mvdrBF");
  if (num_dets < 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "digitalBF / mvdrBF need numDets (digitalBF.m:84, mvdrBF.m:84)");
  return doa_scan(ctx, method, num_dets, ep, Ra, A, nullptr, azi_est, ele_est, cap, n_est);
}

// ------------------------------------------------------------------ UPA angular spectrum / find2DPeaks (include/isac.h)
extern "C" int isac_get_angular_spectrum2d(isac_ctx* ctx, double* p_db, int64_t cap, int32_t dims[2]) {
  ISAC_ENTER(ctx);
  if (ctx->doa2d_rows <= 0 || ctx->doa2d_cols <= 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "no UPA DoA has run on this context");
  if (dims) { dims[0] = ctx->doa2d_rows; dims[1] = ctx->doa2d_cols; }
  if (!p_db) return ISAC_OK;
  const long long n = (long long)ctx->doa2d_rows * ctx->doa2d_cols;
  if (cap < n) return fail(ctx, ISAC_ERR_CAPACITY, "angular spectrum larger than capacity");
  ISAC_TRY(copy_d2h(ctx, p_db, ctx->doa2d_db.p, sizeof(double) * (size_t)n));
  return ISAC_OK;
}

extern "C" int isac_find2d_peaks(isac_ctx* ctx, const double* p_db, int32_t rows, int32_t cols, int32_t n_peaks, int32_t* ele, int32_t* azi,
                                 int32_t* n_found) {
  ISAC_ENTER(ctx);
  if (!p_db || rows <= 0 || cols <= 0 || !n_found || (n_peaks > 0 && (!ele || !azi))) return fail(ctx, ISAC_ERR_INVALID_ARG, "bad arguments");
  *n_found = 0;
  const long long n = (long long)rows * cols;
  if (n > (1ll << 26)) return fail(ctx, ISAC_ERR_INVALID_ARG, "find2DPeaks: matrix too large");
  if (n_peaks <= 0) return fail(ctx, ISAC_ERR_NO_DETECTION, "find2DPeaks needs a positive number of peaks (music.m:69)");
  const int cap = isac_doa2d_peak_cap(rows, cols);
  const size_t map_doubles = ((size_t)n + 1) & ~(size_t)1;                 // (candidates 16-byte aligned behind the map)
  ISAC_TRY(ensure(ctx, ctx->doa2d_user, sizeof(double) * (map_doubles + (size_t)isac_doa2d_cand_doubles(cap))));
  double* d_map = (double*)ctx->doa2d_user.p;
  double* d_cand = d_map + map_doubles;
  ISAC_TRY(copy_h2d(ctx, d_map, p_db, sizeof(double) * (size_t)n));
  ISAC_TRY(isac_doa2d_norm_peaks_dev(ctx, false, d_map, rows, cols, d_cand, cap, nullptr));
  std::vector<int> e, a;
  ISAC_TRY(fetch_select(ctx, nullptr, 0, d_cand, cap, rows, n_peaks, "", e, a));
  for (size_t i = 0; i < e.size(); ++i) { ele[i] = e[i]; azi[i] = a[i]; }
  *n_found = (int)e.size();
  return ISAC_OK;
}

// ------------------------------------------------------------------ music2D (music2D.m:1-123)
extern "C" int isac_music2d_dev(isac_ctx* ctx, const isac_est_params* ep, const isac_music2d_params* mp, const isac_c64* d_rx_grid,
                                const isac_c64* d_tx_grid, int32_t K, int32_t L, int32_t A, isac_est_result* out) {
  ISAC_ENTER(ctx);
  if (!ep || !mp || !d_rx_grid || !d_tx_grid || !out || K <= 0 || L <= 0 || A <= 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "bad arguments");
  std::memset(out, 0, sizeof(*out));
  ctx->last.range_db.clear();                                           // (a call that fails from here on leaves no spectra behind)
  ctx->last.velocity_db.clear();
  const double c0 = 299792458.0;                                        // physconst('LightSpeed')  music2D.m:35
  const double lambda = c0 / mp->fc;                                    // :37
  const double r_gran = 0.5, v_gran = 0.5;                              // :43-44
  const int r_steps = (int)std::floor((mp->r_max + 1.0) / r_gran);      // :45
  const int v_steps = (int)std::floor((mp->v_max + 1.0) / v_gran);      // :46
  // ---- DoA: Ra -> eig -> determineNumTargets -> ULA scan                                   :57-63
  ISAC_TRY(ensure(ctx, ctx->cov, sizeof(c64) * (size_t)std::max(A * A, L * L)));
  ISAC_TRY(isac_covariance_on(ctx, ctx->stream, d_rx_grid, (int64_t)K * L, A, (isac_c64*)ctx->cov.p));
  ISAC_TRY(isac_eigh_dev(ctx, (const c64*)ctx->cov.p, A, nullptr));
  int Lsig = 0;
  ISAC_TRY(num_targets_of_eig(ctx, A, &Lsig));                          // music.m:22
  ISAC_TRY(eig_status(ctx, A));
  out->num_dets = Lsig;
  if (ep->array_is_upa) return fail(ctx, ISAC_ERR_UNSUPPORTED, kUpaRefused);
  int n_steps = 0; const double* d_sind = nullptr;
  ISAC_TRY(get_sind_table(ctx, ep, &d_sind, &n_steps));
  ISAC_TRY(ensure(ctx, ctx->spec, sizeof(double) * (size_t)std::max(n_steps, std::max(r_steps, v_steps))));
  ISAC_TRY(isac_music_scan_dev(ctx, A, nullptr, Lsig, d_sind, n_steps, 0.5, (double*)ctx->spec.p, nullptr));
  std::vector<double>& spec = ctx->last.spectrum_db;                    // the context's last ULA azimuth scan (isac_fft2d_get_music_spectrum)
  spec.resize((size_t)n_steps);
  ISAC_TRY(copy_d2h(ctx, spec.data(), ctx->spec.p, sizeof(double) * (size_t)n_steps));
  ISAC_HIP(hipStreamSynchronize(ctx->stream));
  std::vector<double> azi;
  ISAC_TRY(ula_peaks(ctx, ep, spec, Lsig, "findpeaks 'NPeaks' must be a positive integer", azi));
  out->n_azi = (int)std::min<size_t>(azi.size(), ISAC_MAX_EST);
  doa_store({}, azi, out->n_azi, out->ele_est, out->azi_est);
  // ---- range / velocity: H = channelInfo(:,:,1); Gram matrix G/K = H^H H / K (= conj(Rv));  Rr's signal vectors u = H v / sqrt(K mu)
  ISAC_TRY(ensure(ctx, ctx->stage_a, sizeof(c64) * (size_t)K * L));
  c64* d_h = (c64*)ctx->stage_a.p;
  ISAC_TRY(isac_music2d_plane(ctx, (const c64*)d_rx_grid, (const c64*)d_tx_grid, (long long)K * L, d_h));      // :67-68
  ISAC_TRY(isac_covariance_on(ctx, ctx->stream, (const isac_c64*)d_h, (int64_t)K, L, (isac_c64*)ctx->cov.p));  // G/K        :71-72
  ISAC_TRY(isac_eigh_dev(ctx, (const c64*)ctx->cov.p, L, nullptr));                                            // :77-89
  std::vector<double> wg; std::vector<int> order;
  ISAC_TRY(sorted_eigenpairs(ctx, L, true, wg, nullptr, order));                                                // sort(.,'descend')
  // An empty noise space (Urn / Uvn of :81,:88 have no column: Lsig >= K for the range, Lsig >= L for the velocity) is a flat 0 dB spectrum without
  // estimates, as in the ULA scan (include/isac.h).  H has rank <= L, so Rr has at most L signal vectors whatever Lsig says.
  const bool r_empty = Lsig >= K, v_empty = Lsig >= L;
  const int Lu = std::min(Lsig, L);
  std::vector<int> top(order.begin(), order.begin() + Lu);
  ISAC_TRY(ensure(ctx, ctx->stage_b, sizeof(c64) * (size_t)K * Lu + sizeof(int) * (size_t)Lu + 64));
  c64* d_U = (c64*)ctx->stage_b.p;
  int* d_top = (int*)((char*)ctx->stage_b.p + sizeof(c64) * (size_t)K * Lu);
  ISAC_TRY(copy_h2d(ctx, d_top, top.data(), sizeof(int) * (size_t)Lu));
  std::vector<double> pr((size_t)r_steps, 1.0), pv((size_t)v_steps, 1.0);
  if (!r_empty) {
    ISAC_TRY(isac_music2d_signal_vectors(ctx, d_h, K, L, d_top, Lu, d_U));
    // range scan  ar = exp(-2j*pi*scs*2*r*n/c)                                              :92,:98-102
    const double coef_r = ((-2.0 * M_PI) * mp->scs_hz) * 2.0;
    ISAC_TRY(isac_music2d_scan(ctx, d_U, K, K, nullptr, Lu, 0, coef_r, c0, 0.0, r_gran, r_steps, (double*)ctx->spec.p));
    ISAC_TRY(copy_d2h(ctx, pr.data(), ctx->spec.p, sizeof(double) * (size_t)r_steps));
    ISAC_HIP(hipStreamSynchronize(ctx->stream));
  }
  if (!v_empty) {
    // velocity scan  av = exp(2j*pi*T*2*v*m/lambda), Uvs = conj(V(:,top))                     :93,:104-108
    const double coef_v = ((2.0 * M_PI) * mp->t_sri) * 2.0;
    ISAC_TRY(isac_music2d_scan(ctx, (const c64*)ctx->eig_v.p, L, L, d_top, Lu, 1, coef_v, lambda, -mp->v_max / 2.0, v_gran, v_steps,
                               (double*)ctx->spec.p));
    ISAC_TRY(copy_d2h(ctx, pv.data(), ctx->spec.p, sizeof(double) * (size_t)v_steps));
    ISAC_HIP(hipStreamSynchronize(ctx->stream));
  }
  to_db(pr);                                                            // :111-117
  to_db(pv);
  const std::vector<int> rl = findpeaks_desc(pr, Lsig), vl = findpeaks_desc(pv, Lsig);                          // :120-121
  out->n_rng = (int)std::min<size_t>(rl.size(), ISAC_MAX_EST);
  out->n_vel = (int)std::min<size_t>(vl.size(), ISAC_MAX_EST);
  for (int i = 0; i < out->n_rng; ++i) out->rng_est[i] = rl[(size_t)i] * r_gran;                               // :122
  for (int i = 0; i < out->n_vel; ++i) out->vel_est[i] = vl[(size_t)i] * v_gran - mp->v_max / 2.0;             // :123
  ctx->last.range_db = std::move(pr);                                   // isac_music2d_get_spectra
  ctx->last.velocity_db = std::move(pv);
  return ISAC_OK;
}

extern "C" int isac_music2d_get_spectra(isac_ctx* ctx, double* pr_db, int32_t cap_r, double* pv_db, int32_t cap_v, int32_t n_steps[2]) {
  ISAC_ENTER(ctx);
  const int nr = (int)ctx->last.range_db.size(), nv = (int)ctx->last.velocity_db.size();
  if (nr == 0 && nv == 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "no music2D has completed on this context");
  if (n_steps) { n_steps[0] = nr; n_steps[1] = nv; }
  if (!pr_db && !pv_db) return ISAC_OK;
  if ((pr_db && cap_r < nr) || (pv_db && cap_v < nv)) return fail(ctx, ISAC_ERR_CAPACITY, "music2D spectrum larger than capacity");
  if (pr_db) std::copy(ctx->last.range_db.begin(), ctx->last.range_db.end(), pr_db);
  if (pv_db) std::copy(ctx->last.velocity_db.begin(), ctx->last.velocity_db.end(), pv_db);
  return ISAC_OK;
}
