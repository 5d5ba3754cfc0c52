// C ABI of libisac_hip.so: context, device memory and copies, timers, reserve, options (gfx950 only).
// Declarations and the reference functions each entry point replaces: include/isac.h.
#include <algorithm>
#include <chrono>
#include <map>
#include <mutex>

#include "isac_internal.hpp"

using namespace isac;

// ------------------------------------------------------------------ context
extern "C" int isac_abi_version(void) { return ISAC_ABI_VERSION; }
extern "C" int isac_abi_sizeof(int32_t which) {
  switch (which) {
    case ISAC_SIZEOF_EST_RESULT: return (int)sizeof(isac_est_result);
    case ISAC_SIZEOF_EST_PARAMS: return (int)sizeof(isac_est_params);
    case ISAC_SIZEOF_CFAR_CONFIG: return (int)sizeof(isac_cfar_config);
    case ISAC_SIZEOF_RADAR_CHANNEL_PARAMS: return (int)sizeof(isac_radar_channel_params);
    case ISAC_SIZEOF_CARRIER: return (int)sizeof(isac_carrier);
    case ISAC_SIZEOF_MUSIC2D_PARAMS: return (int)sizeof(isac_music2d_params);
    case ISAC_SIZEOF_CSI_REPORT: return (int)sizeof(isac_csi_report);
    case ISAC_SIZEOF_SENSING_JOB: return (int)sizeof(isac_sensing_job);
    case ISAC_SIZEOF_SRS_REPORT: return (int)sizeof(isac_srs_report);
    case ISAC_SIZEOF_RX_FRONTEND_JOB: return (int)sizeof(isac_rx_frontend_job);
    case ISAC_SIZEOF_PATH_LOSS_CONFIG: return (int)sizeof(isac_path_loss_config);
    case ISAC_SIZEOF_TARGET_LIST: return (int)sizeof(isac_target_list);
    case ISAC_SIZEOF_CFAR_METHOD: return (int)sizeof(isac_cfar_method);
    default: return -1;
  }
}

extern "C" int isac_device_count(int* count) {
  if (!count) return ISAC_ERR_INVALID_ARG;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { *count = 0; return ISAC_ERR_HIP; }
  *count = n;
  return ISAC_OK;
}

extern "C" int isac_ctx_create(int device, isac_ctx** out) {
  if (!out) return ISAC_ERR_INVALID_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return ISAC_ERR_HIP;
  if (hipSetDevice(device) != hipSuccess) return ISAC_ERR_HIP;
  isac_ctx* ctx = new isac_ctx();
  ctx->device = device;
  // the MUSIC branch (covariance -> eigensolver -> scan: the longest dependent chain of a CPI) runs at the highest stream priority:
  // -3 % blocking CPI latency, pipelined rate unchanged
  int prio_lo = 0, prio_hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
  const int p1 = 0, p2 = prio_hi;
  if (hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, p1) != hipSuccess ||
      hipStreamCreateWithPriority(&ctx->stream2, hipStreamNonBlocking, p2) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_cfar, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ctx->ev_done, hipEventDisableTiming) != hipSuccess ||
      hipEventCreate(&ctx->ev_t0) != hipSuccess || hipEventCreate(&ctx->ev_t1) != hipSuccess ||
      hipEventCreate(&ctx->ev_k0) != hipSuccess || hipEventCreate(&ctx->ev_k1) != hipSuccess) {
    delete ctx;
    return ISAC_ERR_HIP;
  }
  ctx->own_stream = ctx->stream;
  ctx->own_stream2 = ctx->stream2;
  *out = ctx;
  return ISAC_OK;
}

extern "C" int isac_ctx_destroy(isac_ctx* ctx) {
  ISAC_ENTER_NOJOIN(ctx);
  // Shared streams (isac_ctx_share_streams) belong to their owner, which may already be gone: never touch them here.  This context's own work
  // is complete when its last submit's completion event has fired (it is recorded behind everything the submit enqueued) and its own streams are idle.
  const bool borrowed = ctx->stream != ctx->own_stream || ctx->stream2 != ctx->own_stream2;
  ctx->stream = ctx->own_stream;
  ctx->stream2 = ctx->own_stream2;
  if (borrowed) (void)hipEventSynchronize(ctx->ev_done);
  (void)hipStreamSynchronize(ctx->stream);
  (void)hipStreamSynchronize(ctx->stream2);
  for (auto& e : ctx->ev_bounce) if (e) (void)hipEventDestroy(e);
  for (auto& e : ctx->ev_tail) if (e) (void)hipEventDestroy(e);
  (void)hipEventDestroy(ctx->ev_fork);
  (void)hipEventDestroy(ctx->ev_join);
  (void)hipEventDestroy(ctx->ev_cfar);
  (void)hipEventDestroy(ctx->ev_done);
  for (auto& sl : ctx->stage_ring)
    if (sl.ev) (void)hipEventDestroy(sl.ev);
  (void)hipEventDestroy(ctx->ev_t0);
  (void)hipEventDestroy(ctx->ev_t1);
  (void)hipEventDestroy(ctx->ev_k0);
  (void)hipEventDestroy(ctx->ev_k1);
  for (hipEvent_t e : ctx->tl)
    if (e) (void)hipEventDestroy(e);
  (void)hipStreamDestroy(ctx->stream);
  (void)hipStreamDestroy(ctx->stream2);
  delete ctx;                                         // every buffer and cached table goes with its owner (DevBuf / PinnedBuf); the context's device is current
  return ISAC_OK;
}

extern "C" const char* isac_last_error(const isac_ctx* ctx) { return ctx ? ctx->err.c_str() : "NULL context"; }

extern "C" int isac_ctx_get_stream(isac_ctx* ctx, void** hip_stream) {
  if (!ctx || !hip_stream) return ISAC_ERR_INVALID_ARG;
  ISAC_ENTER(ctx);
  *hip_stream = (void*)ctx->stream;
  return ISAC_OK;
}

extern "C" int isac_sync(isac_ctx* ctx) {
  ISAC_ENTER(ctx);
  ISAC_HIP(hipStreamSynchronize(ctx->stream));
  ISAC_HIP(hipStreamSynchronize(ctx->stream2));
  return ISAC_OK;
}

// Caller-visible device memory comes from a per-device POOL of blocks the process has allocated before (round 6): isac_dev_free parks a block, isac_dev_alloc hands out the
// smallest parked block that fits (up to 25 % + 64 KB of slack), and only what the pool cannot serve goes to hipMalloc.  A host that allocates per call (the Python tests,
// a MATLAB session creating and clearing handles) then works on memory the process already owns instead of memory fresh from the driver -- see copy_h2d (isac_common.hpp) for
// the fuzz observation behind this -- and saves the ~100 us of a hipMalloc / hipFree pair.  Parked memory is capped (ISAC_DEV_POOL_MB, default 16 384; 0 disables the pool);
// beyond the cap the largest parked block is returned to the driver.
namespace {
struct DevPool {
  std::mutex m;
  std::multimap<size_t, void*> parked[16];
  struct Blk { size_t bytes; bool parked; };
  std::map<void*, Blk> size_of[16];                // every block the pool has handed out or holds
  size_t parked_bytes[16] = {0};
  size_t cap = 16384ull << 20;
  DevPool() { if (const char* e = std::getenv("ISAC_DEV_POOL_MB")) cap = (size_t)std::strtoull(e, nullptr, 10) << 20; }   // configuration (isac.h)
};
DevPool& dev_pool() { static DevPool p; return p; }
}  // namespace
extern "C" int isac_dev_alloc(isac_ctx* ctx, size_t bytes, void** dptr) {
  if (!ctx || !dptr) return ISAC_ERR_INVALID_ARG;
  ISAC_ENTER(ctx);
  DevPool& P = dev_pool();
  const int dev = ctx->device & 15;
  const size_t want = ((bytes ? bytes : 16) + 255) & ~(size_t)255;
  if (P.cap) {
    std::lock_guard<std::mutex> lk(P.m);
    auto it = P.parked[dev].lower_bound(want);
    if (it != P.parked[dev].end() && it->first <= want + want / 4 + 65536) {
      *dptr = it->second;
      P.parked_bytes[dev] -= it->first;
      P.size_of[dev][it->second].parked = false;
      P.parked[dev].erase(it);
      return ISAC_OK;
    }
  }
  ISAC_HIP(hipMalloc(dptr, want));
  if (P.cap) { std::lock_guard<std::mutex> lk(P.m); P.size_of[dev][*dptr] = DevPool::Blk{want, false}; }
  return ISAC_OK;
}
extern "C" int isac_dev_free(isac_ctx* ctx, void* dptr) {
  ISAC_ENTER(ctx);
  if (!dptr) return ISAC_OK;
  ctx->range_cache.touch(dptr, 0);                 // freeing one of the cached grids drops the cached range rows
  ISAC_HIP(hipStreamSynchronize(ctx->stream));
  DevPool& P = dev_pool();
  const int dev = ctx->device & 15;
  if (P.cap) {
    // (hipFree waits for the whole device; a parked block may be handed out again at once, so the same guarantee is kept: nothing on this device still uses it)
    ISAC_HIP(hipDeviceSynchronize());
    std::vector<void*> release;
    {
      std::lock_guard<std::mutex> lk(P.m);
      auto so = P.size_of[dev].find(dptr);
      if (so == P.size_of[dev].end()) { release.push_back(dptr); }                     // not ours (allocated with the pool disabled): straight back to the driver
      else if (so->second.parked) return fail(ctx, ISAC_ERR_INVALID_ARG, "isac_dev_free: this block has been freed already");
      else {
        so->second.parked = true;
        P.parked[dev].emplace(so->second.bytes, dptr);
        P.parked_bytes[dev] += so->second.bytes;
        while (P.parked_bytes[dev] > P.cap && !P.parked[dev].empty()) {                // over the cap: the largest parked block goes back
          auto big = std::prev(P.parked[dev].end());
          P.parked_bytes[dev] -= big->first;
          P.size_of[dev].erase(big->second);
          release.push_back(big->second);
          P.parked[dev].erase(big);
        }
      }
    }
    for (void* r : release) ISAC_HIP(hipFree(r));
    return ISAC_OK;
  }
  ISAC_HIP(hipFree(dptr));
  return ISAC_OK;
}
extern "C" int isac_memcpy_h2d(isac_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes) {
  if (!ctx || (!dst_dev && bytes) || (!src_host && bytes)) return ISAC_ERR_INVALID_ARG;
  ISAC_ENTER(ctx);
  ctx->range_cache.touch(dst_dev, bytes);          // overwriting a cached grid drops the cached range rows
  ISAC_TRY(copy_h2d(ctx, dst_dev, src_host, bytes));
  ISAC_HIP(hipStreamSynchronize(ctx->stream));
  return ISAC_OK;
}
extern "C" int isac_memcpy_d2h(isac_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes) {
  if (!ctx || (!dst_host && bytes) || (!src_dev && bytes)) return ISAC_ERR_INVALID_ARG;
  ISAC_ENTER(ctx);
  ISAC_TRY(copy_d2h(ctx, dst_host, src_dev, bytes));
  ISAC_HIP(hipStreamSynchronize(ctx->stream));
  return ISAC_OK;
}
extern "C" int isac_memcpy_d2d(isac_ctx* ctx, void* dst_dev, const void* src_dev, size_t bytes) {
  if (!ctx || (!dst_dev && bytes) || (!src_dev && bytes)) return ISAC_ERR_INVALID_ARG;
  ISAC_ENTER(ctx);
  ctx->range_cache.touch(dst_dev, bytes);
  ISAC_HIP(hipMemcpyAsync(dst_dev, src_dev, bytes, hipMemcpyDeviceToDevice, ctx->stream));
  return ISAC_OK;
}
extern "C" int isac_memset_dev(isac_ctx* ctx, void* dst_dev, int value, size_t bytes) {
  if (!ctx || (!dst_dev && bytes)) return ISAC_ERR_INVALID_ARG;
  ISAC_ENTER(ctx);
  ctx->range_cache.touch(dst_dev, bytes);
  ISAC_HIP(hipMemsetAsync(dst_dev, value, bytes, ctx->stream));
  return ISAC_OK;
}
extern "C" int isac_timer_start(isac_ctx* ctx) {
  ISAC_ENTER(ctx);
  ISAC_HIP(hipEventRecord(ctx->ev_t0, ctx->stream));
  return ISAC_OK;
}
extern "C" int isac_timer_stop_ms(isac_ctx* ctx, double* elapsed_ms) {
  if (!ctx || !elapsed_ms) return ISAC_ERR_INVALID_ARG;
  ISAC_ENTER(ctx);
  ISAC_HIP(hipEventRecord(ctx->ev_t1, ctx->stream));
  ISAC_HIP(hipEventSynchronize(ctx->ev_t1));
  float ms = 0.f;
  ISAC_HIP(hipEventElapsedTime(&ms, ctx->ev_t0, ctx->ev_t1));
  *elapsed_ms = (double)ms;
  return ISAC_OK;
}

extern "C" int isac_profile_enable(isac_ctx* ctx, int on) {
  ISAC_ENTER(ctx);
  ctx->profile = on != 0;
  ctx->profile_cov = on == 2;
  ctx->profile_recorded = false;
  return ISAC_OK;
}
extern "C" int isac_profile_last_kernel_ms(isac_ctx* ctx, double* ms) {
  ISAC_ENTER(ctx);
  if (!ms) return fail(ctx, ISAC_ERR_INVALID_ARG, "NULL argument");
  if (!ctx->profile || !ctx->profile_recorded) return fail(ctx, ISAC_ERR_INVALID_ARG, "no profiled kernel launch on this context");
  ISAC_HIP(hipEventSynchronize(ctx->ev_k1));
  float f = 0.f;
  ISAC_HIP(hipEventElapsedTime(&f, ctx->ev_k0, ctx->ev_k1));
  *ms = (double)f;
  return ISAC_OK;
}

extern "C" int isac_ctx_reserve(isac_ctx* ctx, int64_t T, int32_t tx_dim_l, const isac_carrier* carrier, const isac_radar_channel_params* rp,
                                const isac_est_params* ep, const isac_cfar_config* cfar, double warm_ms, double* elapsed_ms) {
  ISAC_ENTER(ctx);
  if (!carrier || !rp || !ep || !cfar || T <= 0 || tx_dim_l < 0 || rp->n_ants <= 0 || rp->n_targets <= 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "isac_ctx_reserve: NULL / empty argument");
  if (!std::isfinite(warm_ms) || warm_ms < 0.0) return fail(ctx, ISAC_ERR_INVALID_ARG, "isac_ctx_reserve: warm_ms must be finite and >= 0");   // (NaN / +inf: the dry-run loop would never end)
  if (warm_ms > 5000.0) warm_ms = 5000.0;                                                  // a few seconds at most: 50-300 ms bring the clocks up
  if (ctx->pending.active) return fail(ctx, ISAC_ERR_INVALID_ARG, "isac_ctx_reserve: a submitted fft2D is pending on this context (the dry run would discard it): collect it first");
  const auto t0 = std::chrono::steady_clock::now();
  auto ms_since = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
  int32_t l_whole = 0;
  ISAC_TRY(isac_ofdm_symbol_count(carrier, T, &l_whole));
  const int K = carrier->n_sc, A = rp->n_ants, L = std::max<int>(l_whole, tx_dim_l);
  if (L <= 0) return fail(ctx, ISAC_ERR_SHORT_WAVEFORM, "isac_ctx_reserve: waveform shorter than one OFDM symbol");
  const size_t g_bytes = sizeof(c64) * (size_t)K * L * A, w_bytes = sizeof(c64) * (size_t)T * A;
  DevBuf grid, wave, echo;
  if (ensure(ctx, grid, g_bytes) != ISAC_OK || ensure(ctx, wave, w_bytes) != ISAC_OK || ensure(ctx, echo, g_bytes) != ISAC_OK)
    return fail(ctx, ISAC_ERR_HIP, "isac_ctx_reserve: no device memory for the dry run's grids (T A + 2 K L A elements)");
  void *d_grid = grid.p, *d_wave = wave.p, *d_echo = echo.p;
  std::vector<uint8_t> los((size_t)rp->n_targets, 1);
  int st = isac_synth_qpsk_grid_dev(ctx, (isac_c64*)d_grid, K, L, A, 0x5EEDull, 0);
  if (st == ISAC_OK) st = isac_memset_dev(ctx, d_wave, 0, w_bytes);                     // (rows past the whole symbols stay zero)
  if (st == ISAC_OK && l_whole > 0) st = isac_ofdm_modulate_dev(ctx, (const isac_c64*)d_grid, std::min<int>(l_whole, L), A, carrier, 1.0, (isac_c64*)d_wave, T);
  int n_dry = 0;
  while (st == ISAC_OK) {
    int32_t lo = 0;
    st = isac_mono_static_sensing_fused_dev(ctx, (const isac_c64*)d_wave, T, tx_dim_l, carrier, rp, los.data(), ISAC_NOISE_PHILOX_SPECTRAL, nullptr, 0x5EED0000ull + (uint64_t)n_dry,
                                            (isac_c64*)d_echo, &lo, ep, cfar, (const isac_c64*)d_grid);
    if (st != ISAC_OK) break;
    st = isac_fft2d_submit_cached_dev(ctx, ep, cfar, (const isac_c64*)d_echo, (const isac_c64*)d_grid, K, L, A);
    if (st == ISAC_ERR_INVALID_ARG) st = isac_fft2d_submit_dev(ctx, ep, cfar, (const isac_c64*)d_echo, (const isac_c64*)d_grid, K, L, A);   // (nothing cached: the CUT window left the map)
    if (st != ISAC_OK) break;
    static thread_local isac_est_result res;                                               // (128 KB: not on the stack)
    st = isac_fft2d_collect(ctx, &res);
    if (st == ISAC_ERR_NO_DETECTION || st == ISAC_ERR_CFAR_WINDOW) st = ISAC_OK;          // a dry CPI without estimates has still prepared everything
    ++n_dry;
    if (ms_since() >= warm_ms) break;
  }
  const std::string keep = ctx->err;
  (void)hipStreamSynchronize(ctx->stream);
  (void)hipStreamSynchronize(ctx->stream2);
  ctx->range_cache.valid = false;                                                          // the cached rows belong to grids that are about to be freed
  ctx->last.valid = false;                                                                 // isac_fft2d_get_* must not hand out the dry run's detections / window / Ra
  ctx->last.spectrum_db.clear();                                                           // ... nor its azimuth spectrum (isac_fft2d_get_music_spectrum asks for a scan, not for last.valid)
  ctx->last.range_db.clear(); ctx->last.velocity_db.clear();                               // ... nor, by the same rule, music2D spectra from before the buffers were re-planned (isac_music2d_get_spectra)
  ctx->tgt.drop();                                                                         // nor isac_fft2d_get_targets the dry run's targets
  ctx->profile_recorded = false;                                                           // nor isac_profile_last_kernel_ms the dry run's kernel
  (void)grid.reset(); (void)wave.reset(); (void)echo.reset();
  if (elapsed_ms) *elapsed_ms = ms_since();
  if (st != ISAC_OK) { ctx->err = keep; return st; }
  return ISAC_OK;
}

extern "C" int isac_ctx_set_option(isac_ctx* ctx, int32_t option, int32_t value) {
  ISAC_ENTER(ctx);
  if (value != 0 && value != 1) return fail(ctx, ISAC_ERR_INVALID_ARG, "option values are 0 or 1");
  switch (option) {
    case ISAC_OPT_MUSIC_ROUTE: ctx->music_route = value; return ISAC_OK;          // 0 = signal-subspace eigensolver (default), 1 = full eig
    case ISAC_OPT_TAIL_FUSION: ctx->tail_fusion = value; return ISAC_OK;          // 1 = one Doppler + CFAR launch (default), 0 = separate kernels
    case ISAC_OPT_WIDE_ORDER: ctx->wide_order = value; return ISAC_OK;            // 1 = covariance on the main stream, the narrow kernels on the second
    case ISAC_OPT_CDL_SHARE_SPECTRA: ctx->cdl_share_spectra = value; ctx->os_valid = false; return ISAC_OK;   // 1 = consecutive downlink batches on the same waveforms share their forward transforms
    case ISAC_OPT_UPA_DOA: ctx->upa_doa = value; return ISAC_OK;                  // 1 = UPA DoA through the 2-D scan + find2DPeaks, 0 = ISAC_ERR_UNSUPPORTED
    default: return fail(ctx, ISAC_ERR_INVALID_ARG, "unknown option");
  }
}

// include/isac_lazy_cov.h: the covariance route of a native lazy echo grid, read by the next isac_mono_static_sensing_fused_dev (echo.hip)
extern "C" int isac_ctx_set_lazy_cov_route(isac_ctx* ctx, int32_t route) {
  ISAC_ENTER(ctx);
  if (route != ISAC_LAZY_COV_SPLIT && route != ISAC_LAZY_COV_REGENERATE) return fail(ctx, ISAC_ERR_INVALID_ARG, "lazy covariance route: ISAC_LAZY_COV_SPLIT or ISAC_LAZY_COV_REGENERATE");
  ctx->lazy_cov_route = route;
  return ISAC_OK;
}

extern "C" int isac_ctx_get_lazy_cov_route_used(isac_ctx* ctx, int32_t* route) {
  ISAC_ENTER_NOJOIN(ctx);
  if (!route || ctx->lazy_cov_used < 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "no covariance of a native lazy echo grid on this context yet");
  *route = ctx->lazy_cov_used;
  return ISAC_OK;
}

// Several contexts on ONE pair of streams: a context is then a set of buffers / scratch, and the device executes the calls of all of them
// in submission order -- the wide kernels (beam-sum, fused echo + range, covariance with ISAC_OPT_WIDE_ORDER) one after the other on the main
// stream, never side by side, the narrow ones of each CPI on the second stream underneath.
extern "C" int isac_ctx_share_streams(isac_ctx* ctx, isac_ctx* owner) {
  ISAC_ENTER(ctx);
  if (owner && owner->device != ctx->device) return fail(ctx, ISAC_ERR_INVALID_ARG, "contexts of different devices cannot share streams");
  ISAC_HIP(hipStreamSynchronize(ctx->stream));
  ISAC_HIP(hipStreamSynchronize(ctx->stream2));
  if (ctx->pending.active) return fail(ctx, ISAC_ERR_INVALID_ARG, "a submitted fft2D is pending on this context: collect it first");
  ctx->stream = (owner && owner != ctx) ? owner->stream : ctx->own_stream;
  ctx->stream2 = (owner && owner != ctx) ? owner->stream2 : ctx->own_stream2;
  return ISAC_OK;
}

// ------------------------------------------------------------------ host-pointer wrappers of the echo path
extern "C" int isac_basic_radar_channel(isac_ctx* ctx, const isac_c64* tx_wave, int64_t T,
                                        const isac_radar_channel_params* rp, const uint8_t* los, int noise_mode,
                                        const isac_c64* noise_unit, uint64_t seed, isac_c64* rx_wave) {
  ISAC_ENTER(ctx);
  if (!tx_wave || !rp || !rx_wave || T <= 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "bad arguments");
  const size_t bytes = sizeof(c64) * (size_t)T * rp->n_ants;
  DevBuf d_tx, d_nz, d_rx;                            // (freed on every exit; hipFree waits for the device)
  ISAC_TRY(ensure(ctx, d_tx, bytes));
  ISAC_TRY(ensure(ctx, d_rx, bytes));
  if (noise_mode == ISAC_NOISE_INJECTED && noise_unit) {
    if (ensure(ctx, d_nz, bytes) != ISAC_OK || copy_h2d(ctx, d_nz.p, noise_unit, bytes) != ISAC_OK)
      return fail(ctx, ISAC_ERR_HIP, "noise upload failed");
  }
  if (copy_h2d(ctx, d_tx.p, tx_wave, bytes) != ISAC_OK) return fail(ctx, ISAC_ERR_HIP, "upload failed");
  ISAC_TRY(isac_basic_radar_channel_dev(ctx, (const isac_c64*)d_tx.p, T, rp, los, noise_mode, (const isac_c64*)d_nz.p, seed, (isac_c64*)d_rx.p));
  if (copy_d2h(ctx, rx_wave, d_rx.p, bytes) != ISAC_OK) return fail(ctx, ISAC_ERR_HIP, "download failed");
  return ISAC_OK;
}

extern "C" int isac_mono_static_sensing(isac_ctx* ctx, const isac_c64* tx_wave, int64_t T, int32_t tx_dim_l,
                                        const isac_carrier* carrier, const isac_radar_channel_params* rp, const uint8_t* los,
                                        int noise_mode, const isac_c64* noise_unit, uint64_t seed, isac_c64* echo_grid,
                                        int32_t* l_out) {
  ISAC_ENTER(ctx);
  if (!tx_wave || !rp || !carrier || !echo_grid || T <= 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "bad arguments");
  int32_t lw = 0;
  ISAC_TRY(isac_ofdm_symbol_count(carrier, T, &lw));
  const int L_out = lw < tx_dim_l ? tx_dim_l : lw;
  const size_t wbytes = sizeof(c64) * (size_t)T * rp->n_ants;
  const size_t gbytes = sizeof(c64) * (size_t)carrier->n_sc * (size_t)(L_out > 0 ? L_out : 1) * rp->n_ants;
  DevBuf d_tx, d_nz, d_g;                             // (freed on every exit; hipFree waits for the device)
  ISAC_TRY(ensure(ctx, d_tx, wbytes));
  ISAC_TRY(ensure(ctx, d_g, gbytes));
  if ((noise_mode == ISAC_NOISE_INJECTED || noise_mode == ISAC_NOISE_INJECTED_SPECTRAL) && noise_unit) {
    const size_t nbytes = noise_mode == ISAC_NOISE_INJECTED ? wbytes : gbytes;   // [T x A] samples or [n_sc x L_out x A] grid elements
    if (ensure(ctx, d_nz, nbytes) != ISAC_OK || copy_h2d(ctx, d_nz.p, noise_unit, nbytes) != ISAC_OK)
      return fail(ctx, ISAC_ERR_HIP, "noise upload failed");
  }
  if (copy_h2d(ctx, d_tx.p, tx_wave, wbytes) != ISAC_OK) return fail(ctx, ISAC_ERR_HIP, "upload failed");
  ISAC_TRY(isac_mono_static_sensing_dev(ctx, (const isac_c64*)d_tx.p, T, tx_dim_l, carrier, rp, los, noise_mode,
                                        (const isac_c64*)d_nz.p, seed, (isac_c64*)d_g.p, l_out));
  if (copy_d2h(ctx, echo_grid, d_g.p, gbytes) != ISAC_OK) return fail(ctx, ISAC_ERR_HIP, "download failed");
  return ISAC_OK;
}
