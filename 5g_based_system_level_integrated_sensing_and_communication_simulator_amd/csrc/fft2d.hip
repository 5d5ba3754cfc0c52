// Host side of the fft2D pipeline (gfx950 only): isac_fft2d_submit*_dev / isac_fft2d_collect with the pack kernel between them, the many-cell isac_sensing_submit_n /
// isac_sensing_collect_n, the host-array isac_fft2d and the isac_fft2d_get_* getters of the last call.  Declarations and the reference function of each entry point: include/isac.h.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <numeric>

#include "isac_internal.hpp"

using namespace isac;

namespace {

__global__ void pack_kernel(const int* __restrict__ det_cnt, const int* __restrict__ det_cut, const double* __restrict__ det_pow,
                            const int* __restrict__ num_dets, int A, int cap, int* __restrict__ hdr /* [3 + A+1] */,
                            int* __restrict__ full_cut, double* __restrict__ full_pow, int pack_first,
                            int* __restrict__ first_cut, double* __restrict__ first_pow, const double* __restrict__ spec,
                            int n_steps, double* __restrict__ spec_out, const EighInfo* __restrict__ eig_info) {
  __shared__ int s_off[1025];
  __shared__ int s_cnt[1024];
  const int tid = threadIdx.x;
  for (int a = tid; a < A; a += blockDim.x) s_cnt[a] = det_cnt[a];
  __syncthreads();
  if (tid == 0) {
    int acc = 0, over = 0;
    for (int a = 0; a < A; ++a) {
      s_off[a] = acc;
      int c = s_cnt[a];
      over |= c > cap;
      acc += c < cap ? c : cap;
    }
    s_off[A] = acc;
    hdr[0] = acc;
    hdr[1] = *num_dets;
    hdr[2] = over | ((eig_info && eig_info->status < 0) ? 2 : 0);
  }
  __syncthreads();
  for (int a = tid; a <= A; a += blockDim.x) hdr[3 + a] = s_off[a];
  for (int i = tid; i < n_steps; i += blockDim.x) spec_out[i] = spec[i];
  // flat copy: every thread finds its antenna by binary search, so all loads are issued at once
  const int total = s_off[A];
  for (int o = tid; o < total; o += blockDim.x) {
    int lo = 0, hi = A;                       // largest a with s_off[a] <= o
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (s_off[mid] <= o) lo = mid; else hi = mid;
    }
    const int i = o - s_off[lo];
    const int c = det_cut[(long long)lo * cap + i];
    const double p = det_pow[(long long)lo * cap + i];
    full_cut[o] = c;
    full_pow[o] = p;
    if (o < pack_first) { first_cut[o] = c; first_pow[o] = p; }
  }
}

// ---- the steps of fft2d_submit, in its order.  Argument checks; d_rx_grid == NULL: the echo grid the preceding isac_mono_static_sensing_fused_dev call kept inside the context (d_echo_grid == NULL there): a descriptor the
// covariance kernel re-forms (LazyEcho::native: *d_rx_grid stays NULL), or the context's own buffer
int resolve_grids(isac_ctx* ctx, const isac_est_params* ep, const isac_cfar_config* cfar, const isac_c64** d_rx_grid, const isac_c64* d_tx_grid, int K, int L, int A, bool use_cached_range, bool* lazy_native) {
  if (!ep || !cfar || !d_tx_grid) return fail(ctx, ISAC_ERR_INVALID_ARG, "NULL argument");
  if (!*d_rx_grid) {
    const LazyEcho& lz = ctx->lazy;
    if (!use_cached_range || !lz.valid || lz.K != K || lz.L_out != L || lz.A != A)
      return fail(ctx, ISAC_ERR_INVALID_ARG, "rxGrid is NULL and no lazy echo grid of this shape is held by the context (isac_mono_static_sensing_fused_dev with d_echo_grid == NULL, then isac_fft2d_submit_cached_dev)");
    *lazy_native = lz.native;
    if (!lz.native) *d_rx_grid = (const isac_c64*)ctx->echo_own.p;
  }
  if (A > 1024) return fail(ctx, ISAC_ERR_INVALID_ARG, "bad grid dimensions");   // (pack_kernel's per-antenna counters)
  return check_rdm_dims(ctx, ep, K, L, A);
}
// fft2D.m:106-107 into ctx->cov, on `st`
int enqueue_covariance(isac_ctx* ctx, hipStream_t st, bool lazy_native, const isac_c64* d_rx_grid, int K, int L, int A) {
  timeline_mark(ctx, 4, st);
  if (lazy_native) ISAC_TRY(isac_covariance_lazy_on(ctx, st, (isac_c64*)ctx->cov.p));
  else ISAC_TRY(isac_covariance_on(ctx, st, d_rx_grid, (int64_t)K * L, A, (isac_c64*)ctx->cov.p));
  timeline_mark(ctx, 5, st);
  return ISAC_OK;
}
// per-antenna detection capacity: every CUT of the zone, bounded only by a 256 MB scratch budget (A x cap x 12 B) -- at the default
// zone (8 510 CUTs) and any A <= 2500 an antenna can report every CUT, as phased.CFARDetector2D would
int detection_capacity(const CutWindow& win, int A) { return (int)std::min<long long>(win.n_cut(), std::max<long long>(4096, (256ll << 20) / 12 / A)); }
// pack + one device->host copy on ctx->stream; fills pd.pack and the full-list pointers (pd.doa, pd.first2d: the caller's)
int enqueue_pack(isac_ctx* ctx, int A, int cap, int n_spec, Fft2dPending& pd) {
  const PackLayout& pk = pd.pack = PackLayout::of(A, n_spec);
  const size_t pack_cap = (size_t)A * cap;
  ISAC_TRY(ensure(ctx, ctx->stage_a, pk.first_bytes));
  ISAC_TRY(ensure_pinned(ctx, pk.first_bytes));
  char* dbase = (char*)ctx->stage_a.p;                          // [hdr][spec][pow first][cut first]
  // a second full-size region for the overflow case keeps the fast path one small copy
  ISAC_TRY(ensure(ctx, ctx->stage_b, (sizeof(double) + sizeof(int)) * pack_cap + 64));
  pd.d_ppow_full = (double*)ctx->stage_b.p;
  pd.d_pcut_full = (int*)((char*)ctx->stage_b.p + sizeof(double) * pack_cap);
  hipLaunchKernelGGL(pack_kernel, dim3(1), dim3(256), 0, ctx->stream, (const int*)ctx->det_cnt.p, (const int*)ctx->det_cut.p, (const double*)ctx->det_pow.p, (const int*)ctx->misc.p, A, cap,
                     (int*)dbase, pd.d_pcut_full, pd.d_ppow_full, PackLayout::pack_first, (int*)(dbase + pk.off_cut), (double*)(dbase + pk.off_pow),
                     pd.doa.upa2d ? (const double*)ctx->doa2d_cand.p : (const double*)ctx->spec.p, n_spec, (double*)(dbase + pk.off_spec), pd.doa.refused() ? nullptr : eig_info(ctx, A));
  ISAC_HIP(hipGetLastError());
  ISAC_HIP(hipMemcpyAsync(ctx->pinned.p, dbase, pk.first_bytes, hipMemcpyDeviceToHost, ctx->stream));
  return ISAC_OK;
}

int fft2d_submit(isac_ctx* ctx, const isac_est_params* ep, const isac_cfar_config* cfar, const isac_c64* d_rx_grid, const isac_c64* d_tx_grid, int32_t K, int32_t L, int32_t A, bool use_cached_range) {
  ISAC_ENTER(ctx);
  ctx->pending.active = false;
  bool lazy_native = false;
  ISAC_TRY(resolve_grids(ctx, ep, cfar, &d_rx_grid, d_tx_grid, K, L, A, use_cached_range, &lazy_native));
  ctx->last.valid = false;                                      // before the CPI record can change (Fft2dCpi, isac_common.hpp)
  ctx->tgt.drop();
  const c64 *rx = (const c64*)d_rx_grid, *tx = (const c64*)d_tx_grid;
  // MUSIC branch on the second stream, concurrent with the range-Doppler/CFAR branch:
  //   stream2: covariance (fp64 MFMA) -> eig (one CU)      stream: range IFFT -> Doppler -> CFAR
  ISAC_TRY(ensure(ctx, ctx->cov, sizeof(c64) * (size_t)A * A));
  ISAC_TRY(ensure(ctx, ctx->misc, 512));
  Fft2dPending pd;
  DoaPlan& pl = pd.doa;                                         // tables and every buffer of the DoA tail, before anything is enqueued
  ISAC_TRY(doa_plan(ctx, ep, A, /*mode: MUSIC*/ 0, &pl));
  pd.first2d = std::min(pl.cap2d, 256);                         // UPA: candidates that travel in the result copy; more: a second copy at collect
  const int n_spec = pl.upa2d ? isac_doa2d_cand_doubles(pd.first2d) : pl.n_steps;   // doubles of the pack's spectrum slot: the ULA spectrum, or [counter | first candidates]
  static const bool single_stream = std::getenv("ISAC_SINGLE_STREAM") != nullptr;   // diagnostic: one stream, isolated kernel times
  hipStream_t s2 = single_stream ? ctx->stream : ctx->stream2;
  // ISAC_OPT_WIDE_ORDER: the covariance (a wide kernel) stays on the main stream, behind the echo synthesis / range stage; everything
  // narrow -- Doppler, CFAR, the MUSIC chain, pack, the D2H copy -- runs on the second stream in one sequence.  With contexts that share
  // their streams (isac_ctx_share_streams) the wide kernels of consecutive CPIs then execute back to back, each with the device to itself.
  const bool wide = ctx->wide_order != 0 && !single_stream;
  struct StreamRestore { isac_ctx* c; hipStream_t s; ~StreamRestore() { c->stream = s; } } restore{ctx, ctx->stream};
  auto fork = [&]() -> int { ISAC_HIP(hipEventRecord(ctx->ev_fork, ctx->stream)); ISAC_HIP(hipStreamWaitEvent(s2, ctx->ev_fork, 0)); return ISAC_OK; };
  const bool range_first = wide && !use_cached_range;             // the range stage reads both grids: a wide kernel too
  if (range_first) ISAC_TRY(isac_rdm_power_window(ctx, ep, cfar, rx, tx, K, L, A, false));
  if (!wide) ISAC_TRY(fork());                                    // default order: the second stream branches off before the covariance, wide order: behind it
  ISAC_TRY(enqueue_covariance(ctx, wide ? ctx->stream : s2, lazy_native, d_rx_grid, K, L, A));
  if (wide) { ISAC_TRY(fork()); ctx->stream = s2; }               // (restored on every exit) the calls below enqueue on the second stream
  // music.m:19; nothing for a UPA that collect will refuse; no live replay: collect cannot run the replay time-out recovery before the scan
  auto eig_first_half = [&] { return pl.refused() ? ISAC_OK : doa_eig_first_half(ctx, pl, (const c64*)ctx->cov.p, s2, /*live_replay=*/false); };
  // (wide order: the many-workgroup narrow kernels -- Doppler, CFAR panels, merge -- first, while the next CPI's beam-sum holds the main stream and
  // leaves registers free; the one-workgroup eigensolver kernels then sit under the next fused kernel, where they cost one CU each)
  if (!wide) ISAC_TRY(eig_first_half());
  if (!range_first) ISAC_TRY(isac_rdm_power_window(ctx, ep, cfar, rx, tx, K, L, A, use_cached_range));          // fft2D.m:37-46,61
  const CutWindow win = CutWindow::of(*cfar);                   // what the two range-Doppler calls around this line work on
  const int cap = detection_capacity(win, A);
  ISAC_TRY(isac_cfar_window(ctx, ep, cfar, A, cap));                                         // fft2D.m:62 (+ numDets on device)
  ISAC_HIP(hipEventRecord(ctx->ev_cfar, ctx->stream));
  ISAC_HIP(hipStreamWaitEvent(s2, ctx->ev_cfar, 0));
  if (wide) ISAC_TRY(eig_first_half());
  ISAC_TRY(doa_enqueue(ctx, pl, (const int*)ctx->misc.p, 0, s2));   // numDets comes from the CFAR branch, still on the device   music.m:12
  ISAC_HIP(hipEventRecord(ctx->ev_join, s2));
  ISAC_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
  ISAC_TRY(enqueue_pack(ctx, A, cap, n_spec, pd));
  timeline_mark(ctx, 6, ctx->stream);
  ISAC_HIP(hipEventRecord(ctx->ev_done, ctx->stream));
  ctx->tail_unjoined = wide;                          // (wide order: recorded on the second stream; the main stream joins at this context's next call)
  pd.active = true;                                   // everything the host half and the readers of the last CPI need later
  ctx->pending = pd;
  Fft2dCpi& cpi = ctx->tgt;
  cpi.ep = *ep; cpi.cfar = *cfar; cpi.win = win; cpi.A = A; cpi.L = L; cpi.cap = cap; cpi.d_sind = pl.d_sind; cpi.n_steps = pl.n_steps;
  cpi.state = Fft2dCpi::kSubmitted;
  return ISAC_OK;
}

}  // namespace

extern "C" int isac_fft2d_dev(isac_ctx* ctx, const isac_est_params* ep, const isac_cfar_config* cfar, const isac_c64* d_rx_grid, const isac_c64* d_tx_grid, int32_t K, int32_t L, int32_t A,
                              isac_est_result* out) {
  ISAC_ENTER(ctx);
  if (!out) return fail(ctx, ISAC_ERR_INVALID_ARG, "NULL argument");
  ISAC_TRY(isac_fft2d_submit_dev(ctx, ep, cfar, d_rx_grid, d_tx_grid, K, L, A));
  return isac_fft2d_collect(ctx, out);
}

extern "C" int isac_fft2d_submit_dev(isac_ctx* ctx, const isac_est_params* ep, const isac_cfar_config* cfar,
                                     const isac_c64* d_rx_grid, const isac_c64* d_tx_grid, int32_t K, int32_t L, int32_t A) {
  return fft2d_submit(ctx, ep, cfar, d_rx_grid, d_tx_grid, K, L, A, false);
}
extern "C" int isac_fft2d_submit_cached_dev(isac_ctx* ctx, const isac_est_params* ep, const isac_cfar_config* cfar,
                                            const isac_c64* d_rx_grid, const isac_c64* d_tx_grid, int32_t K, int32_t L, int32_t A) {
  return fft2d_submit(ctx, ep, cfar, d_rx_grid, d_tx_grid, K, L, A, true);
}

// The host half of fft2D.m:63-99 on per-antenna detection lists in CUT order (cut: CUT ordinals cr + n_cut_rows cc, pw: the CUTs' powers, antenna a at
// [ant_off[a], ant_off[a + 1])): det_rc = the 1-based (row, column) pairs, and in `out` the range / velocity estimates, numDets and the detection count.
// num_dets_dev: the device's own count of distinct detected rows, which must agree.
int fft2d_estimates(isac_ctx* ctx, const isac_est_params* ep, const CutWindow& win, int A, const int* ant_off, const std::vector<int>& cut, const std::vector<double>& pw, int num_dets_dev, std::vector<int32_t>& det_rc, isac_est_result* out) {
  const int total = ant_off[A];
  det_rc.resize((size_t)2 * total);
  std::vector<int> all_row, all_col;
  all_row.reserve((size_t)total);
  all_col.reserve((size_t)total);
  std::vector<int> order;
  for (int a = 0; a < A; ++a) {
    const int b = ant_off[a], e = ant_off[a + 1];
    for (int i = b; i < e; ++i) {
      const CutWindow::RowCol rc = win.row_col_of(cut[(size_t)i]);   // 1-based
      det_rc[(size_t)2 * i] = rc.row;
      det_rc[(size_t)2 * i + 1] = rc.col;
    }
    order.resize((size_t)(e - b));
    std::iota(order.begin(), order.end(), b);
    std::stable_sort(order.begin(), order.end(), [&](int p, int q) { return pw[(size_t)p] > pw[(size_t)q]; });   // :89 sort(peaks,'descend')
    for (int i : order) {
      all_row.push_back(det_rc[(size_t)2 * i]);
      all_col.push_back(det_rc[(size_t)2 * i + 1]);
    }
  }
  auto unique_stable = [](const std::vector<int>& v) {      // unique(x,'stable') on the integer bin indices  :99
    std::vector<int> out_;
    std::vector<char> seen;
    for (int x : v) {
      if ((size_t)x >= seen.size()) seen.resize((size_t)x + 1, 0);
      if (!seen[(size_t)x]) { seen[(size_t)x] = 1; out_.push_back(x); }
    }
    return out_;
  };
  const std::vector<int> urow = unique_stable(all_row), ucol = unique_stable(all_col);
  out->total_detections = total;
  out->num_dets = (int)urow.size();                           // :110
  if ((int)urow.size() != num_dets_dev)
    return fail(ctx, ISAC_ERR_HIP, "internal: device numDets disagrees with host unique() count");
  if (urow.size() > ISAC_MAX_EST || ucol.size() > ISAC_MAX_EST)
    return fail(ctx, ISAC_ERR_CAPACITY, "more unique estimates than ISAC_MAX_EST");
  out->n_rng = (int)urow.size();
  out->n_vel = (int)ucol.size();
  for (size_t i = 0; i < urow.size(); ++i) out->rng_est[i] = CutWindow::range_of(urow[i], *ep);
  for (size_t i = 0; i < ucol.size(); ++i) out->vel_est[i] = CutWindow::velocity_of(ucol[i], *ep);
  return ISAC_OK;
}

extern "C" int isac_fft2d_collect(isac_ctx* ctx, isac_est_result* out) {
  ISAC_ENTER_NOJOIN(ctx);                             // (waits for ev_done on the host below: no stream-side join, which would stall a shared main stream)
  if (!out) return fail(ctx, ISAC_ERR_INVALID_ARG, "NULL argument");
  Fft2dPending& pd = ctx->pending;
  if (!pd.active) return fail(ctx, ISAC_ERR_INVALID_ARG, "isac_fft2d_collect without a pending isac_fft2d_submit_dev");
  pd.active = false;
  std::memset(out, 0, sizeof(*out));
  const Fft2dCpi& cpi = ctx->tgt;                     // the CPI that submit recorded: nothing but drop() touches it while one is pending
  const PackLayout& pk = pd.pack;
  const int A = cpi.A;
  char* h = (char*)ctx->pinned.p;
  ISAC_HIP(hipEventSynchronize(ctx->ev_done));      // (not the stream: contexts that share streams have later CPIs queued behind this one)
  ctx->tail_unjoined = false;                       // the narrow chain of this CPI has finished: nothing left for the main stream to wait for
  if (ctx->tl_on) {
    float t[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 7; ++i) (void)hipEventElapsedTime(&t[i], timeline_base(ctx->stream), ctx->tl[i]);
    std::fprintf(stderr, "TL %p B %.1f %.1f E %.1f %.1f C %.1f %.1f T %.1f\n", (void*)ctx, 1e3 * t[0], 1e3 * t[1], 1e3 * t[2], 1e3 * t[3], 1e3 * t[4], 1e3 * t[5], 1e3 * t[6]);
  }
  const int* hdr = (const int*)h;
  const int total = hdr[0];
  const int num_dets_dev = hdr[1];
  if (hdr[2] & 2) return fail(ctx, ISAC_ERR_HIP, "eigensolver did not finish (non-finite covariance, rotation storage exceeded, or an in-launch exchange of the eigensolver timed out)");
  if (hdr[2] & 1) return fail(ctx, ISAC_ERR_CAPACITY, "an antenna produced more CFAR detections than the per-antenna capacity (256 MB of scratch / 12 B / antennas)");
  std::vector<int> cut((size_t)total);
  std::vector<double> pw((size_t)total);
  if (total <= PackLayout::pack_first) {
    std::memcpy(cut.data(), h + pk.off_cut, sizeof(int) * (size_t)total);
    std::memcpy(pw.data(), h + pk.off_pow, sizeof(double) * (size_t)total);
  } else {
    ISAC_TRY(copy_d2h(ctx, cut.data(), pd.d_pcut_full, sizeof(int) * (size_t)total));
    ISAC_TRY(copy_d2h(ctx, pw.data(), pd.d_ppow_full, sizeof(double) * (size_t)total));
  }
  const int* ant_off = hdr + 3;
  Fft2dLast& last = ctx->last;
  last.ant_off.assign(ant_off, ant_off + A + 1);
  last.det_pow = pw;
  ISAC_TRY(fft2d_estimates(ctx, &cpi.ep, cpi.win, A, ant_off, cut, pw, num_dets_dev, last.det_rc, out));
  last.valid = true;
  if (ctx->tgt.state == Fft2dCpi::kSubmitted) ctx->tgt.state = Fft2dCpi::kCollected;   // (dropped in between: a later call rewrote ymid / pwin / the lists)
  last.spectrum_db.clear();
  if (pd.doa.refused()) return fail(ctx, ISAC_ERR_UNSUPPORTED, kUpaRefused);
  // ---- DoA: music.m:94-104 (ULA), :65-71 (UPA) from the pack's spectrum slot
  std::vector<double> ele, azi;
  ISAC_TRY(doa_readout(ctx, pd.doa, &cpi.ep, (const double*)(h + pk.off_spec), pd.first2d, out->num_dets, "no CFAR detection: ", ele, azi));
  out->n_azi = (int)std::min<size_t>(azi.size(), ISAC_MAX_EST);
  doa_store(ele, azi, out->n_azi, out->ele_est, out->azi_est);
  return ISAC_OK;
}

// Many cells' (monoStaticSensing -> fft2D) pairs in two calls: job i on ctxs[i] (include/isac.h).  Nothing here that the single calls do not do -- the point is WHERE the loop
// runs: ~25 launches per job issued back to back from C++ instead of two host-language calls (argument marshalling, ctypes / MEX dispatch) per job.
extern "C" int isac_sensing_submit_n(isac_ctx* const* ctxs, int32_t n, const isac_sensing_job* jobs, int64_t T, int32_t tx_dim_l, const isac_carrier* carrier,
                                     const isac_est_params* ep, const isac_cfar_config* cfar, double pace_us, int32_t* status) {
  if (!ctxs || !jobs || !status || n <= 0 || !carrier || !ep || !cfar || !(pace_us >= 0.0)) return ISAC_ERR_INVALID_ARG;
  for (int i = 0; i < n; ++i) {
    if (!ctxs[i]) return ISAC_ERR_INVALID_ARG;
    for (int j = 0; j < i; ++j)
      if (ctxs[j] == ctxs[i]) return fail(ctxs[i], ISAC_ERR_INVALID_ARG, "isac_sensing_submit_n: a context appears twice (one pending CPI per context)");
  }
  auto t_next = std::chrono::steady_clock::now();
  const auto pace = std::chrono::nanoseconds((long long)(pace_us * 1e3));
  for (int i = 0; i < n; ++i) {
    isac_ctx* c = ctxs[i];
    const isac_sensing_job& jb = jobs[i];
    if (pace_us > 0.0) {
      while (std::chrono::steady_clock::now() < t_next) {}                    // (sub-millisecond spacing: spin, a sleep would overshoot)
      t_next = std::max(t_next, std::chrono::steady_clock::now()) + pace;
    }
    if (c->pending.active) { status[i] = fail(c, ISAC_ERR_INVALID_ARG, "isac_sensing_submit_n: the context still holds a pending CPI (collect it first)"); continue; }
    if (!jb.rp || !jb.d_tx_wave || !jb.d_tx_grid) { status[i] = fail(c, ISAC_ERR_INVALID_ARG, "isac_sensing_submit_n: incomplete job"); continue; }
    int32_t lo = 0;
    int st = isac_mono_static_sensing_fused_dev(c, jb.d_tx_wave, T, tx_dim_l, carrier, jb.rp, jb.los, jb.noise_mode, jb.d_noise_unit, jb.seed, jb.d_echo_grid, &lo, ep, cfar, jb.d_tx_grid);
    if (st == ISAC_OK) {
      const int A = jb.rp->n_ants;
      st = isac_fft2d_submit_cached_dev(c, ep, cfar, jb.d_echo_grid, jb.d_tx_grid, carrier->n_sc, lo, A);
      if (st == ISAC_ERR_INVALID_ARG && jb.d_echo_grid)                        // nothing cached (the CUT window left the map): the plain call reports it
        st = isac_fft2d_submit_dev(c, ep, cfar, jb.d_echo_grid, jb.d_tx_grid, carrier->n_sc, lo, A);
    }
    status[i] = st;
  }
  return ISAC_OK;
}

extern "C" int isac_sensing_collect_n(isac_ctx* const* ctxs, int32_t n, isac_est_result* out, int32_t* status) {
  if (!ctxs || !out || !status || n <= 0) return ISAC_ERR_INVALID_ARG;
  for (int i = 0; i < n; ++i) {
    if (!ctxs[i]) return ISAC_ERR_INVALID_ARG;
    if (!ctxs[i]->pending.active) {                                            // never submitted (status[i] holds why) or already collected
      if (status[i] == ISAC_OK) status[i] = fail(ctxs[i], ISAC_ERR_INVALID_ARG, "isac_sensing_collect_n: no pending CPI on this context");
      std::memset(&out[i], 0, sizeof(out[i]));
      continue;
    }
    status[i] = isac_fft2d_collect(ctxs[i], &out[i]);
  }
  return ISAC_OK;
}

extern "C" int isac_fft2d(isac_ctx* ctx, const isac_est_params* ep, const isac_cfar_config* cfar, const isac_c64* rx_grid,
                          const isac_c64* tx_grid, int32_t K, int32_t L, int32_t A, isac_est_result* out) {
  ISAC_ENTER(ctx);
  if (!rx_grid || !tx_grid) return fail(ctx, ISAC_ERR_INVALID_ARG, "NULL grid");
  const size_t bytes = sizeof(c64) * (size_t)K * L * A;
  DevBuf d_rx, d_tx;
  ISAC_TRY(ensure(ctx, d_rx, bytes));
  ISAC_TRY(ensure(ctx, d_tx, bytes));
  int st = ISAC_OK;
  if (copy_h2d(ctx, d_rx.p, rx_grid, bytes) != ISAC_OK || copy_h2d(ctx, d_tx.p, tx_grid, bytes) != ISAC_OK)      // (on the context's stream and waited for: see copy_h2d)
    st = fail(ctx, ISAC_ERR_HIP, "host->device copy failed");
  if (st == ISAC_OK) st = isac_fft2d_dev(ctx, ep, cfar, (const isac_c64*)d_rx.p, (const isac_c64*)d_tx.p, K, L, A, out);
  (void)hipStreamSynchronize(ctx->stream);            // before the grids go
  return st;
}

extern "C" int isac_fft2d_get_detections(isac_ctx* ctx, int32_t* det_idx, double* det_pow, int32_t cap, int32_t* ant_offsets,
                                         int32_t* n_total) {
  ISAC_ENTER(ctx);
  if (!ctx->last.valid) return fail(ctx, ISAC_ERR_INVALID_ARG, "no completed fft2D call on this context");
  const int total = (int)ctx->last.det_pow.size();
  if (n_total) *n_total = total;
  if (ant_offsets) std::copy(ctx->last.ant_off.begin(), ctx->last.ant_off.end(), ant_offsets);
  if (total > cap) return fail(ctx, ISAC_ERR_CAPACITY, "detection list larger than capacity");
  if (det_idx) std::copy(ctx->last.det_rc.begin(), ctx->last.det_rc.end(), det_idx);
  if (det_pow) std::copy(ctx->last.det_pow.begin(), ctx->last.det_pow.end(), det_pow);
  return ISAC_OK;
}

extern "C" int isac_fft2d_get_power_window(isac_ctx* ctx, double* P, int64_t cap_elems, int32_t dims[3], int32_t* first_row,
                                           int32_t* first_col) {
  ISAC_ENTER(ctx);
  if (!ctx->last.valid) return fail(ctx, ISAC_ERR_INVALID_ARG, "no completed fft2D call on this context");
  const CutWindow& w = ctx->tgt.win;
  if (dims) { dims[0] = w.nr; dims[1] = w.nc; dims[2] = ctx->tgt.A; }
  if (first_row) *first_row = w.first_row;
  if (first_col) *first_col = w.first_col;
  const long long n = (long long)w.nr * w.nc * ctx->tgt.A;
  if (!P) return ISAC_OK;
  if (cap_elems < n) return fail(ctx, ISAC_ERR_CAPACITY, "power window larger than capacity");
  ISAC_TRY(copy_d2h(ctx, P, ctx->pwin.p, sizeof(double) * (size_t)n));
  return ISAC_OK;
}

extern "C" int isac_fft2d_get_covariance(isac_ctx* ctx, isac_c64* Ra, int32_t A) {
  if (!ctx || !Ra) return ISAC_ERR_INVALID_ARG;
  ISAC_ENTER(ctx);
  if (!ctx->last.valid || ctx->tgt.A != A) return fail(ctx, ISAC_ERR_INVALID_ARG, "no completed fft2D call with this A");
  ISAC_TRY(copy_d2h(ctx, Ra, ctx->cov.p, sizeof(c64) * (size_t)A * A));
  return ISAC_OK;
}

extern "C" int isac_fft2d_get_music_spectrum(isac_ctx* ctx, double* p_db, int32_t cap, int32_t* n_steps) {
  ISAC_ENTER(ctx);
  const int n = (int)ctx->last.spectrum_db.size();
  if (n == 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "no ULA azimuth scan has completed on this context");
  if (n_steps) *n_steps = n;
  if (!p_db) return ISAC_OK;
  if (cap < n) return fail(ctx, ISAC_ERR_CAPACITY, "spectrum larger than capacity");
  std::copy(ctx->last.spectrum_db.begin(), ctx->last.spectrum_db.end(), p_db);
  return ISAC_OK;
}

hipEvent_t isac::timeline_base(hipStream_t st) {
  static hipEvent_t base = nullptr;
  if (!base) { (void)hipEventCreate(&base); (void)hipEventRecord(base, st); (void)hipEventSynchronize(base); }
  return base;
}
