// Successive target cancellation on the last completed fft2D (gfx950 only): isac_fft2d_clean_targets (include/isac_clean.h; project-defined).  On a copy R
// of the range rows ymid [nr x L x A], pass after pass:
//   1  P = |rdm|^2 on the power window of R: rdm_window_kernel (beams.hip, the chain of rdm_cell.hpp) + clean_power_kernel
//   2  detector m on every antenna plane: cfar_detect_planes (cfar.hip)          3  hits, sum map, local maxima, order: target_cells_of_planes (targets.hip)
//   4  the first cell                                                            5  its off-grid tone: refine_kernel on R (refine.hip)
//   6  direction: target_scan_snapshots (targets.hip)                            7  parent (host)
//   8  clean_cancel_kernel: the tone's least-squares fit over the active symbols, subtracted from the rows r +- span_rows
// clean_cancel_kernel: one workgroup of 256 threads per row of the span, all rows in one launch.  The fit IS refine_eval (refine_dev.hpp) -- four lanes per antenna, each a
// quarter of the symbols in ascending order, joined (q0 + q1) + (q2 + q3), a second pass of the 64 quads where A > 64 -- on phasors that are zero at the inactive symbols, so
// X_a sums the active ones only; then thread i subtracts (X_a / n_active) conj(p_l) from sample (l, a) = (i % L, i / L) of the row, read and written at stride nr.  The
// phasors, one sincos of the full argument each, are formed once per workgroup and serve the fit and the subtraction.  fp64, no atomics; a workgroup owns its row.
// The loop is host-driven (every pass reads the detector's counts and the first cell back) and recomputes the whole window each pass: off the timed path.
// Steps 4-8 do not depend on how the cell was found: they are cancel_pass, which the loop of isac_fft2d_beam_clean_targets (beam_clean.hip) runs as well; the fit and the
// subtraction are tone_fit_subtract (refine_dev.hpp), which relax_refit_kernel (relax.hip) shares.
#include <cmath>
#include <memory>
#include <vector>

#include "isac_internal.hpp"
#include "refine_dev.hpp"

namespace isac {

__global__ __launch_bounds__(256) void clean_power_kernel(const c64* __restrict__ Y, long long n, double* __restrict__ P) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const c64 y = Y[i];
  P[i] = __dadd_rn(__dmul_rn(y.re, y.re), __dmul_rn(y.im, y.im));          // re^2 + im^2: two rounded products, one rounded sum -- never contracted (as beam_planes_kernel)
}

__global__ __launch_bounds__(256) void clean_cancel_kernel(c64* R /* [nr x L x A] */, int nr, int L, int A, int row_lo /* first window row of the span, 0-based */, double nu,
                                                           const unsigned char* __restrict__ active /* [L] */, double n_active) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  c64* s_ph = reinterpret_cast<c64*>(smem_raw);                           // [L] e^{-2 pi j nu l}, 0 where the symbol is inactive
  c64* s_x = s_ph + L;                                                    // [A]
  double* s_p = reinterpret_cast<double*>(s_x + A);                       // [A]
  double* s_d = s_p + A;                                                  // [A]
  c64* row = R + row_lo + blockIdx.x;                                     // (the host clips the span to 0 .. nr - 1)
  tone_phasors(s_ph, nu, L, active);
  __syncthreads();
  tone_fit_subtract<false>(row, nr, L, A, active, n_active, s_ph, s_x, s_p, s_d);
}

}  // namespace isac

// ================================================================= host side
using namespace isac;

int symbol_mask(isac_ctx* ctx, const char* who, const uint8_t* sym_active, int L, SymbolMask* mask) {
  mask->act.assign((size_t)L, 1);
  mask->n_active = L;
  if (sym_active) {
    mask->n_active = 0;
    for (int l = 0; l < L; ++l) { mask->act[(size_t)l] = sym_active[l] ? 1 : 0; mask->n_active += mask->act[(size_t)l]; }
    if (mask->n_active == 0) return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": sym_active names no active symbol");
  }
  return ISAC_OK;
}

int cancel_pass(isac_ctx* ctx, CancelLoop& s, int row, int col, RowSpan* span, bool* stop) {
  const Fft2dCpi& ts = ctx->tgt;
  const isac_est_params& ep = ts.ep;
  const int A = ts.A, L = ts.L, n_fft = ep.n_fft, i = *s.n_iter;
  // ---- step 4
  s.row[i] = row; s.col[i] = col;
  // ---- steps 5, 6
  const int sel[2] = {row - ts.win.first_row, col - n_fft / 2 - 1};
  ISAC_TRY(stage_upload(ctx, s.d_rec, sel, sizeof(sel)));
  c64* d_snap = s.d_snap + (size_t)A * i;
  ISAC_TRY(refine_enqueue(ctx, s.plan, s.d_R, &s.d_rec->wr, &s.d_rec->k, 1, &s.d_rec->status, &s.d_rec->nu, &s.d_rec->power, d_snap));
  ISAC_TRY(target_scan_snapshots(ctx, d_snap, 1, &s.d_rec->bin, s.azi + i, s.ele ? s.ele + i : nullptr));
  CancelRecord got;
  ISAC_TRY(copy_d2h(ctx, &got, s.d_rec, sizeof(got)));
  s.status[i] = got.status; s.nu[i] = got.nu; s.power[i] = got.power;
  s.vel[i] = got.status == 0 ? got.nu * n_fft * ep.v_res : CutWindow::velocity_of(col, ep);
  s.parent[i] = i;
  *s.n_iter = i + 1;
  *stop = got.status != 0;
  if (*stop) { ++s.kept; return ISAC_OK; }
  // ---- step 7
  s.parent[i] = merge_parent(i, s.row, s.nu, s.parent, nullptr, s.span_rows, s.merge_tol, L);
  s.kept += s.parent[i] == i ? 1 : 0;
  // ---- step 8
  *span = span_of(sel[0], s.span_rows, ts.win.nr);                        // 0 <= sel[0] < nr: a CUT row of the window
  const size_t lds = sizeof(c64) * ((size_t)L + A) + sizeof(double) * 2 * (size_t)A;   // (<= the refinement's, which tone_plan has bounded by 160 KB)
  ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(clean_cancel_kernel), lds));
  hipLaunchKernelGGL(clean_cancel_kernel, dim3(span->len()), dim3(256), lds, ctx->stream, s.d_R, ts.win.nr, L, A, span->lo, got.nu, s.d_act, (double)s.n_active);
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}

int cancel_finish(isac_ctx* ctx, const CancelLoop& s, int32_t* n_kept, isac_c64* snapshots, isac_c64* residual_rows) {
  const Fft2dCpi& ts = ctx->tgt;
  *n_kept = s.kept;
  if (snapshots && *s.n_iter > 0) ISAC_TRY(copy_d2h(ctx, snapshots, s.d_snap, sizeof(c64) * (size_t)ts.A * *s.n_iter));
  if (residual_rows) ISAC_TRY(copy_d2h(ctx, residual_rows, s.d_R, sizeof(c64) * (size_t)ts.win.nr * ts.L * ts.A));
  return ISAC_OK;
}

extern "C" int isac_fft2d_clean_targets(isac_ctx* ctx, const isac_cfar_method* m, int32_t max_iter, int32_t span_rows, double merge_tol, const uint8_t* sym_active, int32_t* n_iter,
                                        int32_t* n_kept, int32_t* n_left, int32_t* row, int32_t* col, int32_t* hits, int32_t* status, int32_t* parent, double* map_power, double* nu,
                                        double* vel, double* rng, double* power, double* azi, double* ele, isac_c64* snapshots, isac_c64* residual_rows) {
  ISAC_ENTER(ctx);
  const char* who = "isac_fft2d_clean_targets";
  if (!m || !n_iter || !n_kept || !n_left || !row || !col || !hits || !status || !parent || !map_power || !nu || !vel || !rng || !power || !azi)
    return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": NULL argument");
  if (max_iter < 1 || max_iter > ISAC_MAX_TARGETS || span_rows < 0 || !std::isfinite(merge_tol) || merge_tol < 0.0)
    return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": max_iter must lie in 1..ISAC_MAX_TARGETS, span_rows and merge_tol must be finite and not negative");
  ISAC_TRY(cpi_ready(ctx, who));
  const Fft2dCpi& ts = ctx->tgt;
  const CutWindow& w = ts.win;
  const int A = ts.A, L = ts.L;
  if (ts.ep.array_is_upa && !ele) return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": a planar array needs ele");
  SymbolMask mask;
  ISAC_TRY(symbol_mask(ctx, who, sym_active, L, &mask));
  ISAC_TRY(needs_halo(ctx, who));
  CancelLoop s{who, {}, nullptr, nullptr, nullptr, nullptr, mask.n_active, span_rows, merge_tol, n_iter, row, col, status, parent, nu, vel, power, azi, ele};
  ISAC_TRY(tone_plan(ctx, who, &s.plan));
  *n_iter = 0; *n_kept = 0; *n_left = 0;
  const long long n_cells = (long long)w.nr * w.nc * A;
  if (n_cells >= (1ll << 31)) return fail(ctx, ISAC_ERR_UNSUPPORTED, std::string(who) + ": the antenna planes hold 2^31 cells or more");
  // one scratch block: [R nr L A | Y nr nc A] c64, [P nr nc A] doubles, the pass's record, the snapshots [A x max_iter], the symbol mask [L]
  const size_t n_rows_el = (size_t)w.nr * L * A;
  Carver cv;
  const size_t off_r = cv.take(sizeof(c64) * n_rows_el), off_y = cv.take(sizeof(c64) * (size_t)n_cells), off_p = cv.take(sizeof(double) * (size_t)n_cells);
  const size_t off_rec = cv.take(sizeof(CancelRecord)), off_snap = cv.take(sizeof(c64) * (size_t)A * max_iter), off_act = cv.take((size_t)L);
  ISAC_TRY(ensure(ctx, ctx->clean, cv.total));
  char* d = (char*)ctx->clean.p;
  s.d_R = (c64*)(d + off_r); s.d_rec = (CancelRecord*)(d + off_rec); s.d_snap = (c64*)(d + off_snap); s.d_act = (const unsigned char*)(d + off_act);
  double* d_P = (double*)(d + off_p);
  ISAC_HIP(hipMemcpyAsync(s.d_R, ctx->ymid.p, sizeof(c64) * n_rows_el, hipMemcpyDeviceToDevice, ctx->stream));
  ISAC_TRY(copy_h2d(ctx, d + off_act, mask.act.data(), (size_t)L));
  std::unique_ptr<isac_target_list> tl(new isac_target_list);
  for (bool stop = false; !stop;) {
    // ---- steps 1-3
    ISAC_TRY(rdm_window_enqueue(ctx, who, s.d_R, (c64*)(d + off_y)));
    hipLaunchKernelGGL(clean_power_kernel, dim3(cdiv(n_cells, 256)), dim3(256), 0, ctx->stream, (const c64*)(d + off_y), n_cells, d_P);
    ISAC_HIP(hipGetLastError());
    PlaneLists pl;
    ISAC_TRY(cfar_detect_planes(ctx, who, m, d_P, A, ctx->clean_det, &pl));
    const PlaneCells src{d_P, A, pl.d_cut, pl.d_cnt, pl.n_cut, false, &ctx->clean_sel, nullptr};
    ISAC_TRY(target_cells_of_planes(ctx, who, src, tl.get()));
    *n_left = tl->n_total;
    const int i = *n_iter;
    if (tl->n_total == 0 || i == max_iter) break;
    // ---- step 4: the first cell; steps 5-8
    hits[i] = tl->hits[0]; map_power[i] = tl->power[0]; rng[i] = tl->rng[0];
    RowSpan span;
    ISAC_TRY(cancel_pass(ctx, s, tl->row[0], tl->col[0], &span, &stop));
  }
  return cancel_finish(ctx, s, n_kept, snapshots, residual_rows);
}
