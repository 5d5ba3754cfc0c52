// Successive target cancellation with the detector on beam planes of the last completed fft2D (gfx950 only): isac_fft2d_beam_clean_targets (include/isac_beam_clean.h;
// project-defined).  On a copy R of the range rows ymid [nr x L x A], pass after pass:
//   1  Y = rdm on the power window of R, Pb = the beam planes of Y and W      2  detector m on every beam plane      3  hits, M = max over the beams, b*, local maxima, order
//   4  the first cell      5  its off-grid tone and direction      6  parent (host)      7  the tone subtracted from the rows r +- span_rows: steps 4-8 of isac_clean.h,
//      cancel_pass (clean.hip)
// The definition recomputes the window in every pass.  Here Pb [nr x nc x B], the per-CUT flags [B x n_cut], M / b* / hits [nr x nc] STAY on the device: pass 0 fills them
// whole with the kernels of isac_fft2d_beam_detect (rdm_window_enqueue, beam_planes_enqueue: beams.hip) and of the detector (cfar_flag_planes: cfar.hip); after a subtraction
// on the window rows lo .. hi only what those rows reach is formed again:
//   K1 beam_band_planes_kernel   rows lo .. hi of Pb from R.  One workgroup per (band row, tile of TC window columns).  Phase 1: Y of the tile, TC x A cells, one cell per
//                                thread and turn by the chain of rdm_cell.hpp straight from R (lanes of one antenna read the same sample: a broadcast), kept in LDS [A][TC].
//                                Phase 2: thread (column, beam group) holds kBeamTile accumulators; the conjugated weights of G kBeamTile beams are staged in LDS in chunks of
//                                AC antennas (ascending, so each accumulator still runs a = 0, 1, ... A - 1), and one LDS read of Y[a] serves the lane's kBeamTile beams.
//                                The cell's expression is beam_planes_kernel's (fma(c64, c64, c64), beam_cell_power: beam_cell.hpp), so the bits are those of a full pass.
//   cfar_flag_planes             the flags of the CUT rows lo - 2 hr .. hi (window rows lo - hr .. hi + hr: the CUTs whose guard + training window meets the band)
//   K2 beam_cell_maps_kernel     M, b* (planes_first_max: beam_cell.hpp) and hits = the number of set flags, on the window rows lo - hr - 1 .. hi + hr + 1; one thread per cell
//   K3 beam_cells_select_kernel  the local-maximum test and the compaction of target_cells_kernel on the maps M and hits, whole: O(nr nc) per pass
// fp64 VALU only (no MFMA: the accumulation order of step 2 is fixed); no floating-point atomics.  The loop is host-driven (every pass reads the candidates back).
#include <algorithm>
#include <cmath>
#include <vector>

#include "isac_internal.hpp"
#include "beam_cell.hpp"
#include "rdm_cell.hpp"

namespace isac {

// ---------------------------------------------------------------- K1
template <int TC>
__global__ __launch_bounds__(256) void beam_band_planes_kernel(const c64* __restrict__ R /* [nr x L x A] */, int nr, int L, int A, int n_fft, const c64* __restrict__ tw_d,
                                                               double sqrt_nfft, int col_first /* rdm column of window column 0, 0-based */, int nc, int row_lo,
                                                               const c64* __restrict__ W /* [A x B] */, const double* __restrict__ norm /* [B] */, int B,
                                                               int AC /* antennas per staged chunk of weights */, double* __restrict__ Pb /* [nr x nc x B] */) {
  constexpr int G = 256 / TC, BT = G * kBeamTile;                         // beam groups per workgroup, beams per step
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  c64* s_y = reinterpret_cast<c64*>(smem_raw);                            // [A][TC]
  c64* s_w = s_y + (size_t)A * TC;                                        // [AC][BT], conjugated
  const int tid = threadIdx.x;
  const int r = row_lo + blockIdx.x, c0 = blockIdx.y * TC;                // (the host clips the band to 0 .. nr - 1)
  for (int i = tid; i < A * TC; i += 256) {
    const int lc = i % TC, a = i / TC;
    const int kbin = rdm_bin_of_column(col_first + min(c0 + lc, nc - 1), n_fft);   // (columns past the window, in the last tile: clamped, never stored)
    const c64* sym = R + r + (long long)nr * L * a;
    const c64 q0 = rdm_cell_quarter(sym, nr, L, n_fft, kbin, 0, tw_d), q1 = rdm_cell_quarter(sym, nr, L, n_fft, kbin, 1, tw_d);
    const c64 q2 = rdm_cell_quarter(sym, nr, L, n_fft, kbin, 2, tw_d), q3 = rdm_cell_quarter(sym, nr, L, n_fft, kbin, 3, tw_d);
    s_y[i] = rdm_cell_join(q0, q1, q2, q3, sqrt_nfft);
  }
  const int lc = tid % TC, g = tid / TC, wc = c0 + lc;
  for (int b0 = 0; b0 < B; b0 += BT) {                                    // (uniform trip counts: every thread reaches every barrier)
    c64 z[kBeamTile];
#pragma unroll
    for (int j = 0; j < kBeamTile; ++j) z[j] = mk(0.0, 0.0);
    for (int a0 = 0; a0 < A; a0 += AC) {                                  // ascending a from 0
      const int na = min(AC, A - a0);
      __syncthreads();                                                    // s_y is complete; the previous chunk's reads of s_w are done
      for (int t = tid; t < na * BT; t += 256) {
        const int al = t % na, j = t / na, b = b0 + j;                    // lanes along a: consecutive c64 of a column of W
        s_w[al * BT + j] = b < B ? conj(W[a0 + al + (long long)A * b]) : mk(0.0, 0.0);
      }
      __syncthreads();
      for (int al = 0; al < na; ++al) {
        const c64 y = s_y[(a0 + al) * TC + lc];
#pragma unroll
        for (int j = 0; j < kBeamTile; ++j) z[j] = fma(s_w[al * BT + g * kBeamTile + j], y, z[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < kBeamTile; ++j) {
      const int b = b0 + g * kBeamTile + j;
      if (b < B && wc < nc) Pb[r + (long long)nr * (wc + (long long)nc * b)] = beam_cell_power(z[j], norm[b]);
    }
  }
}

// ---------------------------------------------------------------- K2: M, b* and hits of the window rows row_lo .. row_lo + n_rows - 1, every column
__global__ __launch_bounds__(256) void beam_cell_maps_kernel(const double* __restrict__ Pb /* [nr x nc x B] */, const unsigned char* __restrict__ flags /* [B][n_cut] */,
                                                             int nr, int nc, int B, int hr, int hc, int n_cut_rows, int n_cut_cols, int row_lo, int n_rows,
                                                             double* __restrict__ M, int* __restrict__ bstar, int* __restrict__ hits /* [nr x nc] each */) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_rows * nc) return;
  const int r = row_lo + i % n_rows, c = i / n_rows;                      // lanes along the rows of the band
  const long long cell = r + (long long)nr * c;
  int best = 0;
  M[cell] = planes_first_max(Pb + cell, (long long)nr * nc, B, &best);
  bstar[cell] = best;
  const int cr = r - hr, cc = c - hc;
  int h = 0;
  if (cr >= 0 && cr < n_cut_rows && cc >= 0 && cc < n_cut_cols) {
    const long long n_cut = (long long)n_cut_rows * n_cut_cols;
    const unsigned char* f = flags + cr + (long long)n_cut_rows * cc;
    for (int b = 0; b < B; ++b) h += f[n_cut * b] != 0 ? 1 : 0;
  }
  hits[cell] = h;
}

// ---------------------------------------------------------------- K3: the test and the compaction of target_cells_kernel on the maps; one thread per CUT cell, rows fastest
struct BeamCand { double m; int cut, hits, plane, pad; };                  // a listed cell: M, CUT ordinal, hits, b* (0-based)
static_assert(sizeof(BeamCand) == 24, "the host copies the candidates as it finds them");

__global__ __launch_bounds__(256) void beam_cells_select_kernel(const double* __restrict__ M, const int* __restrict__ bstar, const int* __restrict__ hits, int nr, int hr, int hc,
                                                                int n_cut_rows, int n_cut, unsigned* __restrict__ count, BeamCand* __restrict__ cand /* [n_cut] */) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  bool tgt = false;
  int h = 0, plane = 0;
  double v = 0.0;
  if (i < n_cut) {
    const int cr = i % n_cut_rows, cc = i / n_cut_rows;
    const long long cell = (hr + cr) + (long long)nr * (hc + cc);        // hr, hc >= 1: all 8 neighbours lie inside the window
    const double* q = M + cell;
    h = hits[cell];
    plane = bstar[cell];
    v = *q;
    // strictly greater than all 8 neighbours: a plateau gives no target, NaN (on either side) compares false
    tgt = h >= 1 && v > q[-nr - 1] && v > q[-nr] && v > q[-nr + 1] && v > q[-1] && v > q[1] && v > q[nr - 1] && v > q[nr] && v > q[nr + 1];
  }
  const unsigned long long mask = __ballot(tgt);
  const int lane = threadIdx.x & 63;
  unsigned base = 0;
  if (lane == 0 && mask) base = atomicAdd(count, (unsigned)__popcll(mask));
  base = __shfl(base, 0);
  if (tgt) {
    const unsigned pos = base + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
    if (pos < (unsigned)n_cut) cand[pos] = BeamCand{v, i, h, plane, 0};   // (a cell is counted once: always true)
  }
}

}  // namespace isac

// ================================================================= host side
using namespace isac;

namespace {

// what stays on the device across the passes, and the geometry of its updates
struct BeamCleanState {
  const char* who;
  const isac_cfar_method* m;
  int B, tc, ac;
  size_t lds_band;
  c64 *d_R, *d_W;
  double *d_Pb, *d_norm, *d_M;
  int *d_bstar, *d_hits;
  unsigned* d_count;                                                        // [count, 16 bytes | BeamCand n_cut]: the list's head leaves in one copy
  unsigned char* d_flags;
};

// K1 on the window rows lo .. hi
int enqueue_band_planes(isac_ctx* ctx, const BeamCleanState& s, int lo, int hi) {
  const Fft2dCpi& ts = ctx->tgt;
  const CutWindow& w = ts.win;
  const int n_fft = ts.ep.n_fft;
  const c64* twd = nullptr;
  ISAC_TRY(isac_get_twiddles(ctx, n_fft, &twd));
#define ISAC_BEAM_BAND(TC_)                                                                                                                                    \
  do {                                                                                                                                                         \
    ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(beam_band_planes_kernel<TC_>), s.lds_band));                                                         \
    hipLaunchKernelGGL(beam_band_planes_kernel<TC_>, dim3(hi - lo + 1, cdiv(w.nc, TC_)), dim3(256), s.lds_band, ctx->stream, (const c64*)s.d_R, w.nr, ts.L, ts.A, \
                       n_fft, twd, std::sqrt((double)n_fft), w.first_col - 1, w.nc, lo, (const c64*)s.d_W, (const double*)s.d_norm, s.B, s.ac, s.d_Pb);        \
  } while (0)
  if (s.tc == 32) ISAC_BEAM_BAND(32); else if (s.tc == 16) ISAC_BEAM_BAND(16); else if (s.tc == 8) ISAC_BEAM_BAND(8); else ISAC_BEAM_BAND(4);
#undef ISAC_BEAM_BAND
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}

// steps 2 and 3 up to the maps, for planes that changed on the window rows lo .. hi (0 .. nr - 1: everything)
int enqueue_flags_and_maps(isac_ctx* ctx, const BeamCleanState& s, int lo, int hi) {
  const CutWindow& w = ctx->tgt.win;
  ISAC_TRY(cfar_flag_planes(ctx, s.who, s.m, s.d_Pb, s.B, lo - 2 * w.hr, hi + 1, s.d_flags));   // the CUT of zone row cr reads the window rows cr .. cr + 2 hr
  const int mlo = std::max(lo - w.hr - 1, 0), mhi = std::min(hi + w.hr + 1, w.nr - 1), n_rows = mhi - mlo + 1;
  hipLaunchKernelGGL(beam_cell_maps_kernel, dim3(cdiv((long long)n_rows * w.nc, 256)), dim3(256), 0, ctx->stream, (const double*)s.d_Pb, (const unsigned char*)s.d_flags, w.nr, w.nc,
                     s.B, w.hr, w.hc, w.n_cut_rows, w.n_cut_cols, mlo, n_rows, s.d_M, s.d_bstar, s.d_hits);
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}

// the rest of step 3: the listed cells in their order -- CUT ordinal, hits, M, b* (0-based) of each
constexpr size_t kCandHead = 170;                                         // candidates fetched with the counter: 16 + 170 x 24 bytes, one page
int list_cells(isac_ctx* ctx, const BeamCleanState& s, std::vector<BeamCand>& cells) {
  const CutWindow& w = ctx->tgt.win;
  const int n_cut = (int)w.n_cut();
  ISAC_HIP(hipMemsetAsync(s.d_count, 0, 16, ctx->stream));
  hipLaunchKernelGGL(beam_cells_select_kernel, dim3(cdiv(n_cut, 256)), dim3(256), 0, ctx->stream, (const double*)s.d_M, (const int*)s.d_bstar, (const int*)s.d_hits, w.nr, w.hr, w.hc,
                     w.n_cut_rows, n_cut, s.d_count, (BeamCand*)((char*)s.d_count + 16));
  ISAC_HIP(hipGetLastError());
  const size_t head = std::min<size_t>(kCandHead, (size_t)n_cut);
  std::vector<char> buf(16 + sizeof(BeamCand) * head);
  ISAC_TRY(copy_d2h(ctx, buf.data(), s.d_count, buf.size()));                // (what lies behind the counted candidates is whatever an earlier pass left: not read)
  unsigned count = 0;
  std::memcpy(&count, buf.data(), sizeof(count));
  if (count > (unsigned)n_cut) return fail(ctx, ISAC_ERR_HIP, "internal: more target cells than CUTs");
  const size_t n = count;
  cells.resize(n);
  if (n == 0) return ISAC_OK;
  std::memcpy(cells.data(), buf.data() + 16, sizeof(BeamCand) * std::min(n, head));
  if (n > head) ISAC_TRY(copy_d2h(ctx, cells.data() + head, (const char*)s.d_count + 16 + sizeof(BeamCand) * head, sizeof(BeamCand) * (n - head)));
  // M descending, ties by ascending column-major index r + nIFFT (c - 1) -- the order of the CUT ordinal (select_cells, targets.hip)
  std::sort(cells.begin(), cells.end(), [](const BeamCand& p, const BeamCand& q) { return p.m != q.m ? p.m > q.m : p.cut < q.cut; });
  return ISAC_OK;
}

}  // namespace

extern "C" int isac_fft2d_beam_clean_targets(isac_ctx* ctx, const isac_c64* W, int32_t n_beams, const double* beam_azi, const isac_cfar_method* m, int32_t max_iter, int32_t span_rows,
                                             double merge_tol, const uint8_t* sym_active, int32_t* n_iter, int32_t* n_kept, int32_t* n_left, int32_t* row, int32_t* col, int32_t* hits,
                                             int32_t* beam, int32_t* status, int32_t* parent, double* map_power, double* nu, double* vel, double* rng, double* power, double* azi,
                                             double* ele, double* beam_label, isac_c64* snapshots, isac_c64* residual_rows, double* beam_pow, int32_t* left_cells) {
  ISAC_ENTER(ctx);
  const char* who = "isac_fft2d_beam_clean_targets";
  if (!W || !m || !n_iter || !n_kept || !n_left || !row || !col || !hits || !beam || !status || !parent || !map_power || !nu || !vel || !rng || !power || !azi || !beam_label)
    return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": NULL argument");
  if (n_beams < 1 || max_iter < 1 || max_iter > ISAC_MAX_TARGETS || span_rows < 0 || !std::isfinite(merge_tol) || merge_tol < 0.0)
    return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": n_beams must be positive, max_iter must lie in 1..ISAC_MAX_TARGETS, span_rows and merge_tol must be finite and not negative");
  ISAC_TRY(cpi_ready(ctx, who));
  const Fft2dCpi& ts = ctx->tgt;
  const isac_est_params& ep = ts.ep;
  const CutWindow& w = ts.win;
  const int A = ts.A, L = ts.L, B = n_beams;
  if (ep.array_is_upa && !ele) return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": a planar array needs ele");
  SymbolMask mask;
  ISAC_TRY(symbol_mask(ctx, who, sym_active, L, &mask));
  const long long n_win = (long long)w.nr * w.nc;
  if (B > ISAC_MAX_BEAMS) return fail(ctx, ISAC_ERR_UNSUPPORTED, std::string(who) + ": more than ISAC_MAX_BEAMS beams");
  if (n_win * B >= (1ll << 31)) return fail(ctx, ISAC_ERR_UNSUPPORTED, std::string(who) + ": the beam planes hold 2^31 cells or more");
  if (n_win * A >= (1ll << 31)) return fail(ctx, ISAC_ERR_UNSUPPORTED, std::string(who) + ": the antenna planes hold 2^31 cells or more");
  ISAC_TRY(needs_halo(ctx, who));
  std::vector<double> norm;
  ISAC_TRY(beam_weight_norms(ctx, who, W, A, B, norm));
  CancelLoop loop{who, {}, nullptr, nullptr, nullptr, nullptr, mask.n_active, span_rows, merge_tol, n_iter, row, col, status, parent, nu, vel, power, azi, ele};
  ISAC_TRY(tone_plan(ctx, who, &loop.plan));
  BeamCleanState s{};
  s.who = who; s.m = m; s.B = B;
  // K1's tile: TC window columns with Y [A x TC] within 64 KB of LDS, the weights of 256 / TC beam groups in chunks of AC antennas within 32 KB
  s.tc = A <= 128 ? 32 : A <= 256 ? 16 : A <= 512 ? 8 : 4;
  if (A > 1024) return fail(ctx, ISAC_ERR_UNSUPPORTED, std::string(who) + ": more than 1024 elements");
  s.ac = std::min(A, 2048 / ((256 / s.tc) * kBeamTile));
  s.lds_band = sizeof(c64) * ((size_t)A * s.tc + (size_t)s.ac * (256 / s.tc) * kBeamTile);
  // one scratch block
  const int n_cut = (int)w.n_cut();
  const size_t n_rows_el = (size_t)w.nr * L * A, n_map = (size_t)n_win;
  Carver cv;
  const size_t off_r = cv.take(sizeof(c64) * n_rows_el), off_y = cv.take(sizeof(c64) * n_map * A), off_w = cv.take(sizeof(c64) * (size_t)A * B), off_snap = cv.take(sizeof(c64) * (size_t)A * max_iter);
  const size_t off_pb = cv.take(sizeof(double) * n_map * B), off_n = cv.take(sizeof(double) * (size_t)B), off_m = cv.take(sizeof(double) * n_map);
  const size_t off_cnt = cv.take(16 + sizeof(BeamCand) * (size_t)n_cut), off_rec = cv.take(sizeof(CancelRecord)), off_bs = cv.take(sizeof(int) * n_map), off_h = cv.take(sizeof(int) * n_map);
  const size_t off_flags = cv.take((size_t)B * n_cut), off_act = cv.take((size_t)L);
  ISAC_TRY(ensure(ctx, ctx->beam_clean, cv.total));
  char* d = (char*)ctx->beam_clean.p;
  s.d_R = (c64*)(d + off_r); s.d_W = (c64*)(d + off_w);
  s.d_Pb = (double*)(d + off_pb); s.d_norm = (double*)(d + off_n); s.d_M = (double*)(d + off_m);
  s.d_bstar = (int*)(d + off_bs); s.d_hits = (int*)(d + off_h);
  s.d_count = (unsigned*)(d + off_cnt); s.d_flags = (unsigned char*)(d + off_flags);
  loop.d_R = s.d_R; loop.d_rec = (CancelRecord*)(d + off_rec); loop.d_snap = (c64*)(d + off_snap); loop.d_act = (const unsigned char*)(d + off_act);
  ISAC_HIP(hipMemcpyAsync(s.d_R, ctx->ymid.p, sizeof(c64) * n_rows_el, hipMemcpyDeviceToDevice, ctx->stream));
  ISAC_TRY(copy_h2d(ctx, s.d_W, W, sizeof(c64) * (size_t)A * B));
  ISAC_TRY(copy_h2d(ctx, s.d_norm, norm.data(), sizeof(double) * (size_t)B));
  ISAC_TRY(copy_h2d(ctx, d + off_act, mask.act.data(), (size_t)L));
  // ---- steps 1-3 of pass 0, whole: the kernels of isac_fft2d_beam_detect and of the detector (a detector block the detector refuses is refused here, before any output)
  ISAC_TRY(rdm_window_enqueue(ctx, who, s.d_R, (c64*)(d + off_y)));
  ISAC_TRY(beam_planes_enqueue(ctx, (const c64*)(d + off_y), n_win, s.d_W, s.d_norm, B, s.d_Pb));
  ISAC_TRY(enqueue_flags_and_maps(ctx, s, 0, w.nr - 1));
  *n_iter = 0; *n_kept = 0; *n_left = 0;
  std::vector<BeamCand> cells;
  for (;;) {
    ISAC_TRY(list_cells(ctx, s, cells));
    *n_left = (int)cells.size();
    const int i = *n_iter;
    if (cells.empty() || i == max_iter) break;
    // ---- step 4: the first cell; steps 5-7
    const BeamCand c0 = cells[0];
    const CutWindow::RowCol rc = w.row_col_of(c0.cut);                    // 1-based
    hits[i] = c0.hits; beam[i] = c0.plane + 1; map_power[i] = c0.m; rng[i] = CutWindow::range_of(rc.row, ep);
    beam_label[i] = beam_azi ? beam_azi[c0.plane] : (double)(c0.plane + 1);
    RowSpan span;
    bool stop = false;
    ISAC_TRY(cancel_pass(ctx, loop, rc.row, rc.col, &span, &stop));
    if (stop) break;
    // ---- steps 1-3 of the next pass on what the band reaches
    ISAC_TRY(enqueue_band_planes(ctx, s, span.lo, span.hi));
    ISAC_TRY(enqueue_flags_and_maps(ctx, s, span.lo, span.hi));
  }
  if (left_cells)
    for (size_t i = 0; i < std::min(cells.size(), (size_t)ISAC_MAX_TARGETS); ++i) {
      const CutWindow::RowCol rc = w.row_col_of(cells[i].cut);
      left_cells[2 * i] = rc.row;
      left_cells[2 * i + 1] = rc.col;
    }
  ISAC_TRY(cancel_finish(ctx, loop, n_kept, snapshots, residual_rows));
  if (beam_pow) ISAC_TRY(copy_d2h(ctx, beam_pow, s.d_Pb, sizeof(double) * n_map * B));
  return ISAC_OK;
}
