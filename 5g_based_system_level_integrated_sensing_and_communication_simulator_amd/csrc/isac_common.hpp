// Shared device/host helpers for libisac_hip (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/isac.h"
#include "cut_window.hpp"
#include "ofdm_symbol.hpp"

namespace isac {

// ---------------------------------------------------------------- complex fp64 (interleaved)
struct __attribute__((aligned(16))) c64 {
  double re, im;
};
static_assert(sizeof(c64) == 16, "c64 must match isac_c64 / MATLAB interleaved complex");

__host__ __device__ inline c64 mk(double r, double i) { return c64{r, i}; }
__host__ __device__ inline c64 operator+(c64 a, c64 b) { return {a.re + b.re, a.im + b.im}; }
__host__ __device__ inline c64 operator-(c64 a, c64 b) { return {a.re - b.re, a.im - b.im}; }
__host__ __device__ inline c64 operator*(c64 a, c64 b) {
  return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
__host__ __device__ inline c64 operator*(c64 a, double s) { return {a.re * s, a.im * s}; }
__host__ __device__ inline c64 operator*(double s, c64 a) { return {a.re * s, a.im * s}; }
__host__ __device__ inline c64 conj(c64 a) { return {a.re, -a.im}; }
__host__ __device__ inline c64 mul_conj(c64 a, c64 b) {  // a * conj(b)
  return {a.re * b.re + a.im * b.im, a.im * b.re - a.re * b.im};
}
__host__ __device__ inline c64 mul_i(c64 a) { return {-a.im, a.re}; }    // * (+j)
__host__ __device__ inline c64 mul_mi(c64 a) { return {a.im, -a.re}; }   // * (-j)
__host__ __device__ inline c64& operator+=(c64& a, c64 b) { a.re += b.re; a.im += b.im; return a; }
__host__ __device__ inline c64 fma(c64 a, c64 b, c64 c) {  // a*b + c
  return {::fma(a.re, b.re, ::fma(-a.im, b.im, c.re)), ::fma(a.re, b.im, ::fma(a.im, b.re, c.im))};
}

// ---------------------------------------------------------------- raw buffer access (bounds-checked by the hardware)
// A buffer descriptor over [base, base + bytes): loads past the end return zero and stores past the end are dropped, so a ragged edge
// needs no branch around the memory instruction (a branch around one makes the compiler's s_waitcnt bookkeeping pessimistic: every
// later wait becomes vmcnt(0)).
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
constexpr int kBufferRsrcFlags = 0x00020000;         // gfx9 raw buffer: DATA_FORMAT = 32 (dword 3 of the descriptor)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_of(const void* base, unsigned bytes) {
  // `base` / `bytes` must be wavefront-uniform.  readfirstlane pins them to scalar registers: a descriptor the compiler cannot prove
  // uniform (e.g. a size that went through a 64-bit VALU multiply) turns every access into a waterfall loop.
  const unsigned long long b = reinterpret_cast<unsigned long long>(base);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
  void* ub = reinterpret_cast<void*>(((unsigned long long)hi << 32) | lo);
  return __builtin_amdgcn_make_buffer_rsrc(ub, 0, (int)__builtin_amdgcn_readfirstlane(bytes), kBufferRsrcFlags);
}
__device__ __forceinline__ c64 buffer_load_c64(__amdgpu_buffer_rsrc_t rs, unsigned byte_off) {
  return __builtin_bit_cast(c64, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)byte_off, 0, 0));
}
__device__ __forceinline__ void buffer_store_c64_nt(__amdgpu_buffer_rsrc_t rs, unsigned byte_off, c64 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), rs, (int)byte_off, 0, /*nt*/ 2);
}

// ---------------------------------------------------------------- context
// Device memory / pinned host memory with one owner: released when the owner goes (a member with its isac_ctx, a local at the end of its scope, a cached table with
// the map that holds it).  Movable, not copyable.  Whoever destroys one has the allocation's device current and nothing in flight that still uses the memory.
template <hipError_t (*Free)(void*)>
struct OwnedBuf {
  void* p = nullptr;
  size_t cap = 0;
  OwnedBuf() = default;
  OwnedBuf(OwnedBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  OwnedBuf& operator=(OwnedBuf&& o) noexcept { if (this != &o) { (void)reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
  OwnedBuf(const OwnedBuf&) = delete;
  OwnedBuf& operator=(const OwnedBuf&) = delete;
  ~OwnedBuf() { (void)reset(); }
  hipError_t reset() {
    const hipError_t e = p ? Free(p) : hipSuccess;
    p = nullptr;
    cap = 0;
    return e;
  }
};
using DevBuf = OwnedBuf<hipFree>;           // sized by ensure()
using PinnedBuf = OwnedBuf<hipHostFree>;    // sized by ensure_pinned_buf()
static_assert(!std::is_copy_constructible<DevBuf>::value && std::is_nothrow_move_constructible<DevBuf>::value, "one owner per allocation");

// What a cached device table is and the parameters it was made for (isac_ctx::tables; cached_table, isac_internal.hpp)
enum TableKind { kTwiddle, kW512Pack, kLogTab, kKaiser3, kKaiser3Shifted, kRiseWindow, kSind, kDoa2d };
struct TableKey {
  TableKind kind;
  std::array<long long, 4> par{};
  bool operator<(const TableKey& o) const { return kind != o.kind ? kind < o.kind : par < o.par; }
};

struct Fft2dLast {  // introspection of the last fft2D call: the host copies (their antennas and window: Fft2dCpi)
  bool valid = false;               // false from every submit (and isac_ctx_reserve) on, true once isac_fft2d_collect has the estimates: the isac_fft2d_get_* calls ask for it, but for the spectrum's
  std::vector<int32_t> det_rc;      // [2 x total] 1-based, CUT order per antenna
  std::vector<double> det_pow;
  std::vector<int32_t> ant_off;     // [A+1]
  std::vector<double> spectrum_db;  // dB spectrum of the context's last ULA azimuth scan, whichever call ran it (doa_readout, isac_music2d_dev); empty: none (isac_fft2d_get_music_spectrum)
  std::vector<double> range_db, velocity_db;  // dB range [r_steps] / velocity [v_steps] spectra of the context's last COMPLETED isac_music2d_dev; both empty: none (isac_music2d_get_spectra)
};

struct RangeCache {  // range rows pre-computed by the fused monoStaticSensing call for the next fft2D
  bool valid = false;
  const void* rx = nullptr;
  const void* tx = nullptr;
  int K = 0, L = 0, A = 0, n_ifft = 0, row_lo = 0, nr = 0;
  void set(const void* rx_, const void* tx_, int K_, int L_, int A_, int n_ifft_, int row_lo_, int nr_) {   // (rx_ == NULL: the native lazy grid)
    *this = RangeCache{true, rx_, tx_, K_, L_, A_, n_ifft_, row_lo_, nr_};
  }
  // a write of [p, p + bytes) through the library (copy, memset, free) that touches either cached grid drops the cache
  void touch(const void* p, size_t bytes) {
    if (!valid) return;
    const size_t g = sizeof(double) * 2 * (size_t)K * (size_t)L * (size_t)A;
    const char *b = (const char*)p, *e = b + (bytes ? bytes : 1);
    auto hits = [&](const void* q) { const char* c = (const char*)q; return c && b < c + g && c < e; };
    if (hits(rx) || hits(tx)) valid = false;
  }
};

// Echo grid that stays inside the context (isac_mono_static_sensing_fused_dev with d_echo_grid == NULL, round 6).  native: the grid is NOT in memory -- it is the function
//   echoGrid[k, l, r] = sum_q D_q[k, l] a_q[r] + sig philox(seed; k, l, r)      (D in ctx->dgrid, a in ctx->steer: the synthesis kernels' own inputs)
// that the covariance kernel of the following isac_fft2d_submit_cached_dev re-forms tile by tile (cov_lazy_kernel) and isac_echo_grid_materialize_dev writes out on request.
// !native: shapes the regenerating kernels do not cover (other carriers / noise modes, A outside 49..64, more than two LoS targets): the grid lives in ctx->echo_own.
struct LazyEcho {
  bool valid = false, native = false;
  int K = 0, L_whole = 0, L_out = 0, A = 0, Q = 0;
  double sig = 0.0;
  unsigned long long seed = 0;
  bool split = false;                      // native, ISAC_LAZY_COV_SPLIT: the noise term's partials (ctx->cov_noise) and the cross partials (ctx->cov_xc) of this grid are in the context
  void set_owned(int K_, int L_, int A_) { *this = LazyEcho{true, false, K_, L_, L_, A_, 0, 0.0, 0}; }      // the grid is in ctx->echo_own
  void set_native(int K_, int L_whole_, int L_out_, int A_, int Q_, double sig_, unsigned long long seed_) { *this = LazyEcho{true, true, K_, L_whole_, L_out_, A_, Q_, sig_, seed_}; }
};

// pinned host -> device parameter staging: a small ring of slots, each guarded by its own event, so that a call's uploads do not wait for the
// previous call's kernels to drain (one slot + one event did: every upload sat in stream order behind whatever was queued before it)
struct StageSlot {
  PinnedBuf mem;
  hipEvent_t ev = nullptr;
  bool busy = false;
};
constexpr int kStageSlots = 128;    // (a batched CDL call stages two or three blocks and a slot is free again only when the stream has REACHED its copy: with 8 slots the host ran 4 calls ahead of the device, with 32 about ten -- 5 ms of config 5's frame; 128: the host issues a frame's applies in 40 ms against 94 ms of GPU work)

struct DoaPlan {  // the direction-finding tail of one covariance: what doa_plan (doa.hip) decides, looks up and sizes before anything is enqueued
  int A = 0, mode = 0;                     // antennas; 0 = MUSIC, 1 = digitalBF, 2 = mvdrBF
  bool upa = false, upa2d = false;         // planar array; ... with ISAC_OPT_UPA_DOA: the 2-D scan + find2DPeaks
  bool sub = false;                        // MUSIC through the signal-subspace eigensolver (the numDets signal vectors are enough: music.m:27-29)
  const double* d_sind = nullptr; int n_steps = 0;   // ULA: sind of the n_steps scan angles
  const double* d_tab2d = nullptr;         // UPA: [sind(ele) e_steps | cosd(azi) a_steps | sind(azi) a_steps], at most cap2d peak candidates
  int e_steps = 0, a_steps = 0, cap2d = 0, n_ants_x = 0, n_ants_y = 0;
  bool refused() const { return upa && !upa2d; }   // music.m:69 without the option
};

// The one description of the context's last CPI, filled once, at the end of a successful fft2d_submit (fft2d.hip).  Readers: isac_fft2d_collect, the getters (under Fft2dLast::valid)
// and -- with the device buffers it describes: ctx->ymid, ctx->pwin, det_cut / det_cnt -- isac_fft2d_get_targets[_upa] (targets.hip) and isac_fft2d_redetect (cfar.hip).
// A submit overwrites the record while the host copies of an OLDER CPI would otherwise still be readable: it clears Fft2dLast::valid (and the pending flag) before anything else,
// and has to keep that order -- a getter must never pair the old lists with the new geometry.  state: are the device buffers still the ones this CPI left?  fft2d_submit sets
// kSubmitted, isac_fft2d_collect promotes that to kCollected, and every function that rewrites one of them calls drop() first -- a later range stage, echo call or submit on the
// context makes the target list ISAC_ERR_INVALID_ARG, never stale.
struct Fft2dCpi {
  enum { kNone = 0, kSubmitted = 1, kCollected = 2 };
  int state = kNone;
  isac_est_params ep{};
  isac_cfar_config cfar{};
  CutWindow win{};                                   // of cfar: the dims of ctx->pwin, the rows of ctx->ymid
  int A = 0, L = 0, cap = 0;                         // antennas, symbols of ymid, per-antenna capacity of det_cut
  const double* d_sind = nullptr; int n_steps = 0;   // MUSIC's ULA scan grid (a cached table of the context)
  void drop() { state = kNone; }
};

// The packed result of a CPI, one device -> host copy of first_bytes: [hdr 3 + A + 1 ints | 16-byte aligned spectrum slot, n_spec doubles | pow first | cut first],
// `first` = the first pack_first detections (more: isac_fft2d_collect fetches the full lists)
struct PackLayout {
  static constexpr int pack_first = 4096;
  size_t off_spec = 0, off_pow = 0, off_cut = 0, first_bytes = 0;
  static PackLayout of(int A, int n_spec) {
    PackLayout p;
    p.off_spec = ((3 + (size_t)A + 1) * sizeof(int) + 15) & ~(size_t)15;
    p.off_pow = p.off_spec + sizeof(double) * (size_t)(n_spec > 0 ? n_spec : 1);
    p.off_cut = p.off_pow + sizeof(double) * (size_t)pack_first; p.first_bytes = p.off_cut + sizeof(int) * (size_t)pack_first;
    return p;
  }
};
struct Fft2dPending {  // state between isac_fft2d_submit_dev and isac_fft2d_collect (the CPI itself: Fft2dCpi)
  bool active = false;
  PackLayout pack;
  int* d_pcut_full = nullptr; double* d_ppow_full = nullptr;   // the full lists on the device, for more than pack_first detections
  DoaPlan doa; int first2d = 0;            // doa.upa2d: the pack's spectrum slot holds [counter | first2d find2DPeaks candidates]
};

}  // namespace isac

struct isac_ctx {
  int device = 0;
  int n_cus = 0;                   // compute units of the device (queried on first use: persistent-grid launches)
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;   // MUSIC branch (covariance/eig) overlaps the RDM branch
  hipStream_t own_stream = nullptr, own_stream2 = nullptr;   // the streams this context created (stream / stream2 may alias another context's: isac_ctx_share_streams)
  hipEvent_t ev_done = nullptr;    // behind the last device operation of isac_fft2d_submit*: what isac_fft2d_collect waits for
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_cfar = nullptr, ev_t0 = nullptr, ev_t1 = nullptr;
  // ISAC_TIMELINE=1 (development aid): timed events around the wide kernels of a CPI, printed by isac_fft2d_collect relative to a
  // process-wide base event -- the device-side schedule of a multi-context pipeline WITHOUT a profiler slowing the host down
  hipEvent_t tl[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // B0 B1 E0 E1 C0 C1 T1
  bool tl_on = false;
  hipEvent_t ev_k0 = nullptr, ev_k1 = nullptr;   // isac_profile_*: around the dominant kernel of the last fused echo call
  bool profile = false, profile_recorded = false;
  bool profile_cov = false;                    // isac_profile_enable(ctx, 2): the event pair brackets the wide covariance launch of fft2D instead of the fused echo kernel
  int lazy_cov_route = 0;          // isac_ctx_set_lazy_cov_route: 0 = split covariance of a native lazy echo grid (noise term beside the beam-sum, default), 1 = the regenerating cov_lazy_kernel
  int lazy_cov_used = -1;          // route the last covariance of a native lazy grid took (isac_ctx_get_lazy_cov_route_used); -1: none yet
  int split_wg = 0;                // workgroup partials the last cov_noise_beam_kernel launch and its cov_noise_tail_kernel left in cov_noise
  hipEvent_t ev_tail[2] = {nullptr, nullptr};   // cov_noise_tail_kernel on the second stream: fork behind the main stream, completion (made on first use)
  bool split_tail_joined = true;   // false: the covariance's reduction has yet to wait for ev_tail[1]
  int music_route = 0;             // ISAC_OPT_MUSIC_ROUTE: 0 = signal-subspace eigensolver for MUSIC (default), 1 = always the full eigendecomposition
  long long eig_epoch = 0;         // launches of eigh_tridiag_dist_kernel on this context (its exchange stamps carry the epoch: no reset between launches)
  bool tail_unjoined = false;      // wide order: ev_done of the last submit has not been waited for by the main stream (ISAC_ENTER joins lazily)
  int wide_order = 0;              // ISAC_OPT_WIDE_ORDER: 1 = fft2D's covariance on the main stream, everything narrow (Doppler, CFAR, MUSIC chain, pack, D2H) on the second
  int tail_fusion = 1;             // ISAC_OPT_TAIL_FUSION: 1 = panel CFAR + per-antenna merge / numDets where applicable (default), 0 = memset + per-antenna CFAR + count
  std::string err;
  std::map<const void*, size_t> lds_allowed;                        // kernel -> dynamic LDS bytes enabled on this context's device
  std::map<isac::TableKey, isac::DevBuf> tables;                    // cached device tables: made on first use, kept until the context goes
  // scratch  (coef [Q x T]: after the fused spectral route with one or two LoS targets only the demodulation windows hold values -- echo.hip prepare_echo, beam_window.hpp)
  isac::DevBuf beam, coef, phase_rx, steer, dgrid, ymid, pwin, flags, det_cut, det_pow, det_cnt, cov_part, cov, cov_noise, cov_xc,
      eig_w, eig_v, eig_scratch, spec, misc, stage_a, stage_b, stage_c, cdl_par, seg, cdl_h, rxfe_tab;
  isac::PinnedBuf pinned;       // results of isac_fft2d_submit* (read by isac_fft2d_collect) -- no other entry point may touch it
  isac::PinnedBuf bounce; hipEvent_t ev_bounce[2] = {nullptr, nullptr};   // pinned bounce buffer of the host-array copies (copy_h2d / copy_d2h)
  isac::PinnedBuf pinned_csi;   // results of isac_csi_report*: its own buffer, so a CSI call between submit and collect cannot clobber a pending CPI
  isac::Fft2dLast last;
  isac::Fft2dPending pending;
  isac::Fft2dCpi tgt;                // the last submitted CPI (named for its first reader, isac_fft2d_get_targets): parameters, window, validity of ymid / pwin / det_*
  isac::DevBuf tgt_scratch;          // ... and its device scratch (hits map, candidate lists, snapshots)
  isac::DevBuf tgt_part;             // isac_fft2d_get_targets_upa: per (scan tile, target) partial maxima of the 2-D Bartlett scan, sized once the target count is known
  isac::DevBuf redet;                // isac_fft2d_redetect (cfar.hip): per-CUT flags, per-antenna lists sized for every CUT, counts, row flags
  isac::DevBuf beam_y, beam_p, beam_det, beam_sel;   // isac_fft2d_get_rdm_window / isac_fft2d_beam_detect (beams.hip): complex window [nr x nc x A] (+ W), beam planes [nr x nc x B], the detector's scratch, the cells'
  isac::DevBuf refine;               // isac_fft2d_refine_targets (refine.hip): the cells, their status / scan bin / nu / power, the refined snapshots [A x n]
  isac::DevBuf clean, clean_det, clean_sel;   // isac_fft2d_clean_targets (clean.hip): [residual rows | complex window] c64, the power planes, the pass's record (CancelRecord), the snapshots, the symbol mask -- carved by isac::Carver (cpi_post.hpp), as the next two are; the detector's scratch, the cells'
  isac::DevBuf beam_clean;           // isac_fft2d_beam_clean_targets (beam_clean.hip): [residual rows | complex window | W | snapshots] c64, [beam planes | n_b | M] doubles, [count | the listed cells' records], the pass's record (CancelRecord), b*, hits, the per-CUT flags [B x n_cut], the symbol mask
  isac::DevBuf relax;                // isac_fft2d_relax_targets (relax.hip): [residual rows | tone amplitudes n x span x A | snapshots] c64, [nu | previous nu | power], the entries' rows, spans and schedule, the symbol mask
  isac::DevBuf directions;           // isac_resolve_directions (directions.hip): the snapshots [A x n], the sources' amplitudes and directions [K x n], residuals, counts
  isac::DevBuf cancel_paths;         // isac_cancel_paths_dev (cancel_paths.hip): the Gram pass's partial tiles and power partials, [G | B] and C, the subtract pass's power partials, the status record
  isac::DevBuf range_refine;         // isac_range_refine_dev (range_refine.hip): a chunk's contracted planes [16][A][K] and Doppler phasors [L x 16], the chunk's nu / rows, the entries' status / rho / power / snapshots
  isac::DevBuf cfar_mc;            // isac_cfar_monte_carlo (cfar.hip): detection counts, per-trial flags
  isac::RangeCache range_cache;
  isac::LazyEcho lazy;               // the echo grid of the last fused monoStaticSensing call when the caller passed no array for it
  // overlap-save CDL apply (cdl_os.hip): the forward spectra of the last downlink batch, kept in a buffer of their own so that the NEXT batch on this context can reuse them when
  // ISAC_OPT_CDL_SHARE_SPECTRA is set and it names the same waveforms (the UEs of a cell receive one waveform whatever their delay profile: uePhy.m:724-731)
  isac::DevBuf os_x;
  std::vector<const void*> os_waves;
  long long os_T = 0; int os_nt = 0, os_mpad = 0, os_tb = 0; bool os_valid = false;
  int cdl_share_spectra = 0;
  isac::DevBuf echo_own;             // ... and its storage when it has to exist in memory (LazyEcho::native == false)
  // ISAC_OPT_UPA_DOA (doa2d.hip): the 2-D (elevation x azimuth) scan of a UPA
  int upa_doa = 0;                   // 0 = UPA DoA returns ISAC_ERR_UNSUPPORTED (default), 1 = 2-D scan + find2DPeaks
  isac::DevBuf doa2d_p, doa2d_db, doa2d_cand, doa2d_w, doa2d_user;  // raw spectrum, dB map, peak candidates, eigen weights, a caller's map
  int doa2d_rows = 0, doa2d_cols = 0;   // dims of the dB map in doa2d_db (0: none yet)
  isac::StageSlot stage_ring[isac::kStageSlots];   // pinned->device parameter uploads (stage_acquire / stage_commit)
  int stage_next = 0;
  isac::DevBuf localize;             // isac_position_map_dev / isac_localize_dev (localize.hip): the scene's tables, the blocks' candidate lists [blocks][256], the candidates, the outputs' device copies
  isac::DevBuf track;                // isac_track_step_dev (track.hip): [nodes | links | the banks' group ranges | the groups | the measurements], one staged upload; assoc, assoc_kind [M], n_confirmed [B]
};

namespace isac {

inline int fail(isac_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  return code;
}

// Dynamic LDS above the 64 KB default has to be enabled per kernel and per device; remembered in the context (a
// process-wide flag would miss a second device).
inline int allow_lds(isac_ctx* ctx, const void* kernel, size_t bytes) {
  size_t& have = ctx->lds_allowed[kernel];
  if (have < bytes) {
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return fail(ctx, ISAC_ERR_HIP, std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") + hipGetErrorString(e));
    have = bytes;
  }
  return ISAC_OK;
}

#define ISAC_HIP(call)                                                                     \
  do {                                                                                     \
    hipError_t e__ = (call);                                                               \
    if (e__ != hipSuccess)                                                                 \
      return isac::fail(ctx, ISAC_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e__)); \
  } while (0)

// Top of every extern "C" entry point that takes a context: NULL check + make the context's device current on the
// calling thread (scratch allocations, table uploads and hipFuncSetAttribute all act on the CURRENT device, so a
// process that holds contexts on several GPUs, or uses a context from a thread other than its creator, must switch).
#define ISAC_ENTER_NOJOIN(ctx)                                                                     \
  do {                                                                                             \
    if (!(ctx)) return ISAC_ERR_INVALID_ARG;                                                       \
    if (hipSetDevice((ctx)->device) != hipSuccess)                                                 \
      return isac::fail((ctx), ISAC_ERR_HIP, "hipSetDevice failed for the context's device");     \
  } while (0)
#define ISAC_ENTER(ctx)                                                                            \
  do {                                                                                             \
    ISAC_ENTER_NOJOIN(ctx);                                                                        \
    if ((ctx)->tail_unjoined) {                                                                    \
      /* ISAC_OPT_WIDE_ORDER: the previous CPI's narrow chain (Doppler .. D2H) sits on the second  \
         stream and the main stream was never joined behind it; the next call on THIS context       \
         may overwrite ymid / cov / beam / the result buffers that chain still reads */             \
      (ctx)->tail_unjoined = false;                                                                \
      if (hipStreamWaitEvent((ctx)->stream, (ctx)->ev_done, 0) != hipSuccess)                       \
        return isac::fail((ctx), ISAC_ERR_HIP, "hipStreamWaitEvent failed");                       \
    }                                                                                              \
  } while (0)

#define ISAC_TRY(call)              \
  do {                              \
    int s__ = (call);               \
    if (s__ != ISAC_OK) return s__; \
  } while (0)

inline int ensure(isac_ctx* ctx, DevBuf& b, size_t bytes) {
  if (b.cap >= bytes && b.p) return ISAC_OK;
  if (b.p) {
    ISAC_HIP(hipStreamSynchronize(ctx->stream));
    if (const hipError_t e = b.reset()) return fail(ctx, ISAC_ERR_HIP, std::string("hipFree(b.p): ") + hipGetErrorString(e));
  }
  size_t want = bytes < 256 ? 256 : bytes;
  ISAC_HIP(hipMalloc(&b.p, want));
  b.cap = want;
  return ISAC_OK;
}

inline int ensure_pinned_buf(isac_ctx* ctx, PinnedBuf& b, size_t bytes) {
  if (b.cap >= bytes) return ISAC_OK;
  ISAC_HIP(b.reset());
  ISAC_HIP(hipHostMalloc(&b.p, bytes, hipHostMallocDefault));
  b.cap = bytes;
  return ISAC_OK;
}
inline int ensure_pinned(isac_ctx* ctx, size_t bytes) {
  if (ctx->pinned.cap >= bytes) return ISAC_OK;
  if (ctx->pinned.p && ctx->ev_done) ISAC_HIP(hipEventSynchronize(ctx->ev_done));   // a submitted CPI's D2H copy may still be writing the old buffer
  return ensure_pinned_buf(ctx, ctx->pinned, bytes);
}

// Host -> device copy that is COMPLETE when it returns and ordered in front of everything enqueued on the context's streams afterwards.  hipMemcpy on the NULL stream
// returns once a PAGEABLE source has been staged -- its DMA may still be in flight -- and the context's streams are non-blocking (no implicit synchronisation with the NULL
// stream): a kernel launched on them right away could read the destination before the data has landed.  Seen once in ~4 700 fuzz cases under 16 concurrent processes
// (the |rdm|^2 window of a host-array fft2D call off by 1e-2, profiles/r05_fuzz_campaigns.txt); the copy therefore runs ON the context's stream and is waited for.
// Round 6: no PAGEABLE host memory is handed to the runtime any more.  Caller arrays (MATLAB / NumPy memory) go through a pinned bounce buffer of the context in 8 MB chunks,
// two in flight: memcpy into the chunk, hipMemcpyAsync from it on the context's stream, one synchronisation at the end.  The fuzz campaigns of rounds 5-6 under 16
// concurrent processes saw ~1 case in 250 in which a kernel read a (partly) ZERO channel estimate right after the estimate had been uploaded into freshly allocated
// device memory from a pageable array and the stream had been synchronised (profiles/r06_fuzz_campaigns.txt); the runtime's own staging of pageable copies and the
// driver's handling of fresh allocations are the two things such a case passes through that the hot path (pinned buffers, memory allocated once) never does.
constexpr size_t kBounceChunk = 8u << 20;
inline int bounce_ready(isac_ctx* ctx, size_t bytes) {
  const size_t want = bytes < kBounceChunk ? (bytes < 4096 ? 4096 : bytes) : 2 * kBounceChunk;
  if (ctx->bounce.cap < want) {
    ISAC_HIP(hipStreamSynchronize(ctx->stream));
    ISAC_TRY(ensure_pinned_buf(ctx, ctx->bounce, want));
  }
  for (auto& e : ctx->ev_bounce) if (!e) ISAC_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return ISAC_OK;
}
inline int copy_h2d(isac_ctx* ctx, void* dst, const void* src, size_t bytes) {           // complete when it returns
  if (!bytes) return ISAC_OK;
  ISAC_TRY(bounce_ready(ctx, bytes));
  bool used[2] = {false, false};
  int half = 0;
  for (size_t off = 0; off < bytes; off += kBounceChunk, half ^= 1) {
    const size_t n = bytes - off < kBounceChunk ? bytes - off : kBounceChunk;
    char* b = (char*)ctx->bounce.p + (ctx->bounce.cap >= 2 * kBounceChunk ? (size_t)half * kBounceChunk : 0);
    if (used[half]) ISAC_HIP(hipEventSynchronize(ctx->ev_bounce[half]));          // the chunk's previous copy has left the bounce buffer
    std::memcpy(b, (const char*)src + off, n);
    ISAC_HIP(hipMemcpyAsync((char*)dst + off, b, n, hipMemcpyHostToDevice, ctx->stream));
    ISAC_HIP(hipEventRecord(ctx->ev_bounce[half], ctx->stream));
    used[half] = true;
  }
  ISAC_HIP(hipStreamSynchronize(ctx->stream));
  return ISAC_OK;
}
inline int copy_d2h(isac_ctx* ctx, void* dst, const void* src, size_t bytes) {           // waits for the stream first: everything enqueued before is in the copy
  if (!bytes) return ISAC_OK;
  ISAC_TRY(bounce_ready(ctx, bytes));
  const bool two = ctx->bounce.cap >= 2 * kBounceChunk;
  size_t pend_off[2] = {0, 0}, pend_n[2] = {0, 0};
  int half = 0;
  for (size_t off = 0; off < bytes; off += kBounceChunk, half ^= 1) {
    const size_t n = bytes - off < kBounceChunk ? bytes - off : kBounceChunk;
    const int h = two ? half : 0;
    char* b = (char*)ctx->bounce.p + (size_t)h * kBounceChunk;
    if (pend_n[h]) { ISAC_HIP(hipEventSynchronize(ctx->ev_bounce[h])); std::memcpy((char*)dst + pend_off[h], b, pend_n[h]); pend_n[h] = 0; }
    ISAC_HIP(hipMemcpyAsync(b, (const char*)src + off, n, hipMemcpyDeviceToHost, ctx->stream));
    ISAC_HIP(hipEventRecord(ctx->ev_bounce[h], ctx->stream));
    pend_off[h] = off; pend_n[h] = n;
  }
  ISAC_HIP(hipStreamSynchronize(ctx->stream));
  for (int h = 0; h < 2; ++h) if (pend_n[h]) std::memcpy((char*)dst + pend_off[h], (char*)ctx->bounce.p + (size_t)h * kBounceChunk, pend_n[h]);
  return ISAC_OK;
}

inline int upload(isac_ctx* ctx, DevBuf& b, const void* src, size_t bytes) {            // size b, then copy_h2d into it
  ISAC_TRY(ensure(ctx, b, bytes));
  ISAC_TRY(copy_h2d(ctx, b.p, src, bytes));           // (not hipMemcpy: see copy_h2d)
  return ISAC_OK;
}

// Small host block -> device scratch through the context's pinned staging ring: asynchronous, no stream synchronisation; the host waits only when the
// ring wraps onto a slot whose copy has not left it yet.  stage_acquire hands out the next slot's host memory, stage_commit enqueues its copy.
inline int stage_acquire(isac_ctx* ctx, size_t bytes, void** host) {
  StageSlot& sl = ctx->stage_ring[ctx->stage_next];
  if (!sl.ev) ISAC_HIP(hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
  if (sl.busy) { ISAC_HIP(hipEventSynchronize(sl.ev)); sl.busy = false; }    // the slot's previous upload has left it
  if (sl.mem.cap < bytes) ISAC_TRY(ensure_pinned_buf(ctx, sl.mem, bytes < 65536 ? 65536 : bytes));
  *host = sl.mem.p;
  return ISAC_OK;
}
inline int stage_commit(isac_ctx* ctx, void* d_dst, size_t bytes) {
  StageSlot& sl = ctx->stage_ring[ctx->stage_next];
  ISAC_HIP(hipMemcpyAsync(d_dst, sl.mem.p, bytes, hipMemcpyHostToDevice, ctx->stream));
  ISAC_HIP(hipEventRecord(sl.ev, ctx->stream));
  sl.busy = true;
  ctx->stage_next = (ctx->stage_next + 1) % kStageSlots;
  return ISAC_OK;
}
inline int stage_upload(isac_ctx* ctx, void* d_dst, const void* src, size_t bytes) {
  void* h = nullptr;
  ISAC_TRY(stage_acquire(ctx, bytes, &h));
  std::memcpy(h, src, bytes);
  return stage_commit(ctx, d_dst, bytes);
}
// Several small host arrays -> ONE staged upload into a device scratch buffer: add() appends an array and returns its byte offset (a multiple of `align`),
// upload() sizes the buffer and enqueues the copy.
struct MetaPack {
  size_t align;
  std::vector<char> host;
  explicit MetaPack(size_t align_ = 64) : align(align_) {}
  size_t add(const void* src, size_t bytes) {
    const size_t off = host.size();
    host.resize(off + (bytes + align - 1) / align * align, 0);
    if (bytes) std::memcpy(host.data() + off, src, bytes);
    return off;
  }
  template <class T>
  size_t add(const std::vector<T>& v) { return add(v.data(), sizeof(T) * v.size()); }
  int upload(isac_ctx* ctx, DevBuf& b) {
    ISAC_TRY(ensure(ctx, b, host.size() + 64));
    return stage_upload(ctx, b.p, host.data(), host.size());
  }
};

// isac_profile_*: the event pair around the launch(es) a call wants timed
inline int profile_begin(isac_ctx* ctx) {
  if (ctx->profile) ISAC_HIP(hipEventRecord(ctx->ev_k0, ctx->stream));
  return ISAC_OK;
}
inline int profile_end(isac_ctx* ctx) {
  if (ctx->profile) { ISAC_HIP(hipEventRecord(ctx->ev_k1, ctx->stream)); ctx->profile_recorded = true; }
  return ISAC_OK;
}

// compute units of the context's device (queried once: the persistent-grid launches size themselves by it)
inline int ctx_n_cus(isac_ctx* ctx, int* n_cus) {
  if (ctx->n_cus <= 0) {
    int v = 0;
    ISAC_HIP(hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, ctx->device));
    ctx->n_cus = v > 0 ? v : 256;
  }
  *n_cus = ctx->n_cus;
  return ISAC_OK;
}

// (OFDM numerology -- Numerology, numerology, cp_of_symbol, symbol_start: ofdm_symbol.hpp)

// host-side launch geometry helper
inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

}  // namespace isac
