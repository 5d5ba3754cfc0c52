// Beamformed detection on the last completed fft2D (gfx950 only): isac_fft2d_get_rdm_window and isac_fft2d_beam_detect (include/isac_beams.h; project-defined, DESIGN.md
// section 5).  fft2D detects on every antenna plane by itself; here the array is combined coherently BEFORE the detector:
//   1  Y[r, c, a] = rdm(r, c, a) on every cell of the power window, from the range rows ymid [nr x L x A] -- the chain of rdm_cell.hpp, the one target_snapshot runs
//   2  Z[r, c, b] = sum_a conj(W[a, b]) Y[r, c, a] (ascending a, fp64 FMAs), Pb = |Z|^2 / n_b, n_b = sum_a |W[a, b]|^2 (host)
//   3  detector m on every beam plane: cfar_detect_planes (cfar.hip), the device code of isac_fft2d_redetect
//   4  hits = beams whose list holds the cell, M = max_b Pb, target = CUT cell with hits >= 1 and M strictly above its 8 neighbours: target_cells_of_planes (targets.hip)
// K1 rdm_window_kernel: one workgroup per (tile of R window rows, antenna).  The tile's R x L range samples are loaded ONCE into LDS (lanes along the window row: ymid is
// row-fastest, so a wave reads consecutive c64) and serve all nc columns; thread (row, column group) then runs the per-cell chain for its columns out of LDS.
// K2 beam_planes_kernel: one lane per cell (lanes along the flattened window: consecutive c64 of an antenna plane), kBeamTile beams per workgroup with their conjugated
// weights [A x kBeamTile] in LDS (every lane reads the same word: a broadcast), kBeamTile accumulators in registers.  Plain fp64 VALU; both kernels are off the timed path.
#include <algorithm>
#include <cmath>

#include "isac_internal.hpp"
#include "beam_cell.hpp"
#include "rdm_cell.hpp"

namespace isac {

__global__ __launch_bounds__(256) void rdm_window_kernel(const c64* __restrict__ ymid /* [nr x L x A] */, int nr, int L, int n_fft, const c64* __restrict__ tw_d, double sqrt_nfft,
                                                         int col_first /* rdm column of window column 0, 0-based */, int nc, int R /* rows per tile: a power of two <= 64 */,
                                                         c64* __restrict__ Y /* [nr x nc x A] */) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  c64* s_y = reinterpret_cast<c64*>(smem_raw);                            // [L][R], rows fastest
  const int tid = threadIdx.x, a = blockIdx.y, r0 = blockIdx.x * R;
  const c64* src = ymid + (long long)nr * L * a;
  for (int i = tid; i < R * L; i += 256) {
    const int lr = i % R, l = i / R;
    s_y[i] = src[min(r0 + lr, nr - 1) + (long long)nr * l];              // (rows past the window, in the last tile: clamped, never used)
  }
  __syncthreads();
  const int lr = tid % R, g = tid / R, G = 256 / R;
  const int r = r0 + lr;
  if (r >= nr) return;
  for (int wc = g; wc < nc; wc += G) {
    const int kbin = rdm_bin_of_column(col_first + wc, n_fft);
    const c64 q0 = rdm_cell_quarter(s_y + lr, R, L, n_fft, kbin, 0, tw_d), q1 = rdm_cell_quarter(s_y + lr, R, L, n_fft, kbin, 1, tw_d);
    const c64 q2 = rdm_cell_quarter(s_y + lr, R, L, n_fft, kbin, 2, tw_d), q3 = rdm_cell_quarter(s_y + lr, R, L, n_fft, kbin, 3, tw_d);
    Y[r + (long long)nr * (wc + (long long)nc * a)] = rdm_cell_join(q0, q1, q2, q3, sqrt_nfft);
  }
}

__global__ __launch_bounds__(256) void beam_planes_kernel(const c64* __restrict__ Y /* [n_cells x A] */, long long n_cells, int A, const c64* __restrict__ W /* [A x B] */,
                                                          const double* __restrict__ norm /* [B]: n_b */, int B, double* __restrict__ Pb /* [n_cells x B] */) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  c64* s_w = reinterpret_cast<c64*>(smem_raw);                            // [A][kBeamTile], conjugated
  const int tid = threadIdx.x, b0 = blockIdx.y * kBeamTile;
  const int nb = min(kBeamTile, B - b0);
  for (int t = tid; t < A * kBeamTile; t += 256) {
    const int j = t % kBeamTile, a = t / kBeamTile;
    s_w[t] = j < nb ? conj(W[a + (long long)A * (b0 + j)]) : mk(0.0, 0.0);
  }
  __syncthreads();
  const long long i = (long long)blockIdx.x * 256 + tid;
  if (i >= n_cells) return;
  c64 z[kBeamTile];
#pragma unroll
  for (int j = 0; j < kBeamTile; ++j) z[j] = mk(0.0, 0.0);
  for (int a = 0; a < A; ++a) {                                           // ascending a from 0
    const c64 y = Y[i + n_cells * a];
#pragma unroll
    for (int j = 0; j < kBeamTile; ++j) z[j] = fma(s_w[a * kBeamTile + j], y, z[j]);
  }
#pragma unroll
  for (int j = 0; j < kBeamTile; ++j)
    if (j < nb) Pb[i + n_cells * (b0 + j)] = beam_cell_power(z[j], norm[b0 + j]);   // beam_cell.hpp: re^2 + im^2 as two rounded products and one rounded sum, never contracted
}

}  // namespace isac

// ================================================================= host side
using namespace isac;

int cpi_ready(isac_ctx* ctx, const char* who) {
  if (!ctx->last.valid || ctx->tgt.state != Fft2dCpi::kCollected)
    return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": no completed fft2D on this context whose range rows are still on the device");
  return ISAC_OK;
}

int needs_halo(isac_ctx* ctx, const char* who) {
  if (ctx->tgt.win.hr < 1 || ctx->tgt.win.hc < 1)
    return fail(ctx, ISAC_ERR_UNSUPPORTED, std::string(who) + ": the local-maximum test needs a halo of at least one cell (guard + training) in both dimensions");
  return ISAC_OK;
}

namespace {

// step 1 into ctx->beam_y
int enqueue_rdm_window(isac_ctx* ctx, const char* who) {
  const CutWindow& w = ctx->tgt.win;
  ISAC_TRY(ensure(ctx, ctx->beam_y, sizeof(c64) * (size_t)w.nr * w.nc * ctx->tgt.A));
  return rdm_window_enqueue(ctx, who, (const c64*)ctx->ymid.p, (c64*)ctx->beam_y.p);
}

}  // namespace

int rdm_window_enqueue(isac_ctx* ctx, const char* who, const c64* d_rows, c64* d_Y) {
  const Fft2dCpi& ts = ctx->tgt;
  const CutWindow& w = ts.win;
  const int A = ts.A, L = ts.L, n_fft = ts.ep.n_fft;
  int R = 32;                                                             // rows per tile: the tile [L x R] c64 within 64 KB of LDS
  while (R > 1 && sizeof(c64) * (size_t)R * L > 64 * 1024) R >>= 1;
  const size_t lds = sizeof(c64) * (size_t)R * L;                          // (R was halved until the tile fits the 64 KB every kernel may take: no allow_lds)
  if (lds > 64 * 1024) return fail(ctx, ISAC_ERR_UNSUPPORTED, std::string(who) + ": more than 4096 symbols");
  const c64* twd = nullptr;
  ISAC_TRY(isac_get_twiddles(ctx, n_fft, &twd));
  hipLaunchKernelGGL(rdm_window_kernel, dim3(cdiv(w.nr, R), A), dim3(256), lds, ctx->stream, d_rows, w.nr, L, n_fft, twd, std::sqrt((double)n_fft), w.first_col - 1, w.nc, R, d_Y);
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}

int beam_weight_norms(isac_ctx* ctx, const char* who, const isac_c64* W, int A, int B, std::vector<double>& norm) {
  norm.resize((size_t)B);
  for (int b = 0; b < B; ++b) {                                           // n_b in fp64, ascending a from 0.0
    double n = 0.0;
    for (int a = 0; a < A; ++a) { const isac_c64& v = W[a + (size_t)A * b]; n += v.re * v.re + v.im * v.im; }
    if (!(n > 0.0) || !std::isfinite(n)) return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": a column of W has a zero or non-finite norm");
    norm[(size_t)b] = n;
  }
  return ISAC_OK;
}

int beam_planes_enqueue(isac_ctx* ctx, const c64* d_Y, long long n_cells, const c64* d_W, const double* d_norm, int B, double* d_Pb) {
  const int A = ctx->tgt.A;
  const size_t lds = sizeof(c64) * (size_t)A * kBeamTile;
  ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(beam_planes_kernel), lds));
  hipLaunchKernelGGL(beam_planes_kernel, dim3(cdiv(n_cells, 256), cdiv(B, kBeamTile)), dim3(256), lds, ctx->stream, d_Y, n_cells, A, d_W, d_norm, B, d_Pb);
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}

extern "C" int isac_fft2d_get_rdm_window(isac_ctx* ctx, isac_c64* Y, int64_t cap_elems, int32_t dims[3], int32_t* first_row, int32_t* first_col) {
  ISAC_ENTER(ctx);
  ISAC_TRY(cpi_ready(ctx, "isac_fft2d_get_rdm_window"));
  const CutWindow& w = ctx->tgt.win;
  if (dims) { dims[0] = w.nr; dims[1] = w.nc; dims[2] = ctx->tgt.A; }
  if (first_row) *first_row = w.first_row;
  if (first_col) *first_col = w.first_col;
  const long long n = (long long)w.nr * w.nc * ctx->tgt.A;
  if (!Y) return ISAC_OK;
  if (cap_elems < n) return fail(ctx, ISAC_ERR_CAPACITY, "complex window larger than capacity");
  ISAC_TRY(enqueue_rdm_window(ctx, "isac_fft2d_get_rdm_window"));
  ISAC_TRY(copy_d2h(ctx, Y, ctx->beam_y.p, sizeof(c64) * (size_t)n));
  return ISAC_OK;
}

extern "C" int isac_fft2d_beam_detect(isac_ctx* ctx, const isac_c64* W, int32_t n_beams, const double* beam_azi, const isac_cfar_method* m, isac_target_list* out, int32_t* beam,
                                      int32_t* det_idx, double* det_pow, int32_t cap, int32_t* beam_offsets, int32_t* n_total, double* beam_pow) {
  ISAC_ENTER(ctx);
  const char* who = "isac_fft2d_beam_detect";
  if (!W || !m || !out || !beam || n_beams < 1 || cap < 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "bad arguments");
  ISAC_TRY(cpi_ready(ctx, who));
  const Fft2dCpi& ts = ctx->tgt;
  const CutWindow& w = ts.win;
  const int A = ts.A, B = n_beams;
  const long long n_cells = (long long)w.nr * w.nc;
  if (B > ISAC_MAX_BEAMS) return fail(ctx, ISAC_ERR_UNSUPPORTED, std::string(who) + ": more than ISAC_MAX_BEAMS beams");
  if (n_cells * B >= (1ll << 31)) return fail(ctx, ISAC_ERR_UNSUPPORTED, std::string(who) + ": the beam planes hold 2^31 cells or more");
  ISAC_TRY(needs_halo(ctx, who));
  std::vector<double> norm;
  ISAC_TRY(beam_weight_norms(ctx, who, W, A, B, norm));
  // ---- steps 1, 2: ctx->beam_y = [Y nr nc A | W A B | n_b B], ctx->beam_p = the beam planes
  Carver cv;
  const size_t off_y = cv.take(sizeof(c64) * (size_t)n_cells * A), off_w = cv.take(sizeof(c64) * (size_t)A * B), off_n = cv.take(sizeof(double) * (size_t)B);   // (off_y = 0: where enqueue_rdm_window writes)
  ISAC_TRY(ensure(ctx, ctx->beam_y, cv.total));
  ISAC_TRY(ensure(ctx, ctx->beam_p, sizeof(double) * (size_t)n_cells * B));
  char* dy = (char*)ctx->beam_y.p;
  ISAC_TRY(copy_h2d(ctx, dy + off_w, W, sizeof(c64) * (size_t)A * B));
  ISAC_TRY(copy_h2d(ctx, dy + off_n, norm.data(), sizeof(double) * (size_t)B));
  ISAC_TRY(enqueue_rdm_window(ctx, who));                                  // (beam_y is large enough already: ensure keeps it)
  ISAC_TRY(beam_planes_enqueue(ctx, (const c64*)(dy + off_y), n_cells, (const c64*)(dy + off_w), (const double*)(dy + off_n), B, (double*)ctx->beam_p.p));
  // ---- step 3: the detector of isac_fft2d_redetect on the beam planes
  PlaneLists pl;
  ISAC_TRY(cfar_detect_planes(ctx, who, m, (const double*)ctx->beam_p.p, B, ctx->beam_det, &pl));
  std::memset(out, 0, sizeof(*out));
  if (n_total) *n_total = pl.total();
  if (beam_offsets) std::copy(pl.off.begin(), pl.off.end(), beam_offsets);
  if (pl.total() > cap) return fail(ctx, ISAC_ERR_CAPACITY, "detection list larger than capacity");
  if (det_idx || det_pow) {
    std::vector<int> cut;
    std::vector<double> pw;
    ISAC_TRY(cfar_fetch_lists(ctx, pl, cut, pw));
    if (det_idx)
      for (size_t i = 0; i < cut.size(); ++i) {
        const CutWindow::RowCol rc = w.row_col_of(cut[i]);                 // 1-based
        det_idx[2 * i] = rc.row;
        det_idx[2 * i + 1] = rc.col;
      }
    if (det_pow) std::copy(pw.begin(), pw.end(), det_pow);
  }
  if (beam_pow) ISAC_TRY(copy_d2h(ctx, beam_pow, ctx->beam_p.p, sizeof(double) * (size_t)n_cells * B));
  // ---- step 4: hits, M = max over the beams, local maxima, order
  const PlaneCells src{(const double*)ctx->beam_p.p, B, pl.d_cut, pl.d_cnt, pl.n_cut, true, &ctx->beam_sel, beam};
  ISAC_TRY(target_cells_of_planes(ctx, who, src, out));
  const int n = std::min(out->n_total, (int)ISAC_MAX_TARGETS);
  for (int i = 0; i < n; ++i) {
    out->azi[i] = beam_azi ? beam_azi[beam[i]] : (double)(beam[i] + 1);
    beam[i] += 1;                                                          // 1-based
  }
  out->n_targets = n;
  return ISAC_OK;
}
