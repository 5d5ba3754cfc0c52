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
  const int tid = threadIdx.x;
  c64* row = R + row_lo + blockIdx.x;                                     // (the host clips the span to 0 .. nr - 1)
  for (int l = tid; l < L; l += 256) s_ph[l] = active[l] ? refine_phasor(nu, l) : mk(0.0, 0.0);
  __syncthreads();
  (void)refine_eval(row, nr, L, A, s_ph, s_x, s_p, s_d);                  // s_x[a] = sum over the active symbols; ends with a barrier: every read of the row is done
  for (int i = tid; i < L * A; i += 256) {
    const int l = i % L, a = i / L;
    if (!active[l]) continue;
    const c64 c = mk(s_x[a].re / n_active, s_x[a].im / n_active);
    c64* y = row + (long long)nr * (l + (long long)L * a);
    *y = *y - c * conj(s_ph[l]);
  }
}

}  // namespace isac

// ================================================================= host side
using namespace isac;

int clean_cancel_enqueue(isac_ctx* ctx, c64* d_R, int row_lo, int row_hi, double nu, const unsigned char* d_active, int n_active) {
  const Fft2dCpi& ts = ctx->tgt;
  const size_t lds = sizeof(c64) * ((size_t)ts.L + ts.A) + sizeof(double) * 2 * (size_t)ts.A;   // (<= the refinement's, which refine_plan has bounded by 160 KB)
  ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(clean_cancel_kernel), lds));
  hipLaunchKernelGGL(clean_cancel_kernel, dim3(row_hi - row_lo + 1), dim3(256), lds, ctx->stream, d_R, ts.win.nr, ts.L, ts.A, row_lo, nu, d_active, (double)n_active);
  ISAC_HIP(hipGetLastError());
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
  if (!ctx->last.valid || ctx->tgt.state != Fft2dCpi::kCollected)       // the rule of isac_fft2d_get_targets
    return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": no completed fft2D on this context whose range rows are still on the device");
  const Fft2dCpi& ts = ctx->tgt;
  const isac_est_params& ep = ts.ep;
  const CutWindow& w = ts.win;
  const int A = ts.A, L = ts.L, n_fft = ep.n_fft;
  if (ep.array_is_upa && !ele) return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": a planar array needs ele");
  std::vector<unsigned char> act((size_t)L, 1);
  int n_active = L;
  if (sym_active) {
    n_active = 0;
    for (int l = 0; l < L; ++l) { act[(size_t)l] = sym_active[l] ? 1 : 0; n_active += act[(size_t)l]; }
    if (n_active == 0) return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": sym_active names no active symbol");
  }
  if (w.hr < 1 || w.hc < 1) return fail(ctx, ISAC_ERR_UNSUPPORTED, std::string(who) + ": the local-maximum test needs a halo of at least one cell (guard + training) in both dimensions");
  RefinePlan plan;
  ISAC_TRY(refine_plan(ctx, who, &plan));
  if (ep.array_is_upa) {                                                   // n_ants_x n_ants_y != A: ISAC_ERR_INVALID_ARG; A > 256: ISAC_ERR_UNSUPPORTED -- before any work
    const double* d_tab = nullptr;
    int e_steps = 0, a_steps = 0;
    ISAC_TRY(isac_doa2d_grid(ctx, &ep, A, &d_tab, &e_steps, &a_steps));
  }
  *n_iter = 0; *n_kept = 0; *n_left = 0;
  // one scratch block: [R nr L A | Y nr nc A] c64, [P nr nc A] doubles, the pass's record [window row | k | status | scan bin] ints, [nu | power] doubles, the snapshots
  // [A x max_iter], the symbol mask [L]
  const long long n_cells = (long long)w.nr * w.nc * A;
  if (n_cells >= (1ll << 31)) return fail(ctx, ISAC_ERR_UNSUPPORTED, std::string(who) + ": the antenna planes hold 2^31 cells or more");
  const size_t n_rows_el = (size_t)w.nr * L * A;
  const size_t off_y = sizeof(c64) * n_rows_el, off_p = off_y + sizeof(c64) * (size_t)n_cells, off_rec = (off_p + sizeof(double) * (size_t)n_cells + 15) & ~(size_t)15;
  const size_t off_nu = off_rec + 16, off_snap = off_nu + 16, off_act = off_snap + sizeof(c64) * (size_t)A * max_iter;
  ISAC_TRY(ensure(ctx, ctx->clean, off_act + (size_t)L));
  char* d = (char*)ctx->clean.p;
  c64* d_R = (c64*)d;
  double* d_P = (double*)(d + off_p);
  int* d_rec = (int*)(d + off_rec);
  ISAC_HIP(hipMemcpyAsync(d_R, ctx->ymid.p, sizeof(c64) * n_rows_el, hipMemcpyDeviceToDevice, ctx->stream));
  ISAC_TRY(copy_h2d(ctx, d + off_act, act.data(), (size_t)L));
  std::unique_ptr<isac_target_list> tl(new isac_target_list);
  int kept = 0;
  for (int i = 0;; ++i) {
    // ---- steps 1-3
    ISAC_TRY(rdm_window_enqueue(ctx, who, d_R, (c64*)(d + off_y)));
    hipLaunchKernelGGL(clean_power_kernel, dim3(cdiv(n_cells, 256)), dim3(256), 0, ctx->stream, (const c64*)(d + off_y), n_cells, d_P);
    ISAC_HIP(hipGetLastError());
    PlaneLists pl;
    ISAC_TRY(cfar_detect_planes(ctx, who, m, d_P, A, ctx->clean_det, &pl));
    const PlaneCells src{d_P, A, pl.d_cut, pl.d_cnt, pl.n_cut, false, &ctx->clean_sel, nullptr};
    ISAC_TRY(target_cells_of_planes(ctx, who, src, tl.get()));
    *n_left = tl->n_total;
    if (tl->n_total == 0 || i == max_iter) break;
    // ---- step 4
    row[i] = tl->row[0]; col[i] = tl->col[0]; hits[i] = tl->hits[0]; map_power[i] = tl->power[0]; rng[i] = tl->rng[0];
    // ---- steps 5, 6
    const int sel[2] = {row[i] - w.first_row, col[i] - n_fft / 2 - 1};
    ISAC_TRY(stage_upload(ctx, d_rec, sel, sizeof(sel)));
    c64* d_snap = (c64*)(d + off_snap) + (size_t)A * i;
    ISAC_TRY(refine_enqueue(ctx, plan, d_R, d_rec, d_rec + 1, 1, d_rec + 2, (double*)(d + off_nu), (double*)(d + off_nu) + 1, d_snap));
    ISAC_TRY(target_scan_snapshots(ctx, d_snap, 1, d_rec + 3, azi + i, ele ? ele + i : nullptr));
    double np[2];
    ISAC_TRY(copy_d2h(ctx, status + i, d_rec + 2, sizeof(int)));
    ISAC_TRY(copy_d2h(ctx, np, d + off_nu, sizeof(np)));
    nu[i] = np[0]; power[i] = np[1];
    vel[i] = status[i] == 0 ? nu[i] * n_fft * ep.v_res : CutWindow::velocity_of(col[i], ep);
    parent[i] = i;
    *n_iter = i + 1;
    if (status[i] != 0) { ++kept; break; }
    // ---- step 7 (merge_tol == 0: every entry is kept)
    if (merge_tol != 0.0)
      for (int k = 0; k < i; ++k)
        if (parent[k] == k && std::abs(row[i] - row[k]) <= span_rows && std::fabs(nu[i] - nu[k]) * L <= merge_tol) { parent[i] = k; break; }
    kept += parent[i] == i ? 1 : 0;
    // ---- step 8
    const int wr = sel[0];                                                 // 0 <= wr < nr: a CUT row of the window
    const int lo = (int)std::max<long long>((long long)wr - span_rows, 0), hi = (int)std::min<long long>((long long)wr + span_rows, w.nr - 1);
    ISAC_TRY(clean_cancel_enqueue(ctx, d_R, lo, hi, nu[i], (const unsigned char*)(d + off_act), n_active));
  }
  *n_kept = kept;
  if (snapshots && *n_iter > 0) ISAC_TRY(copy_d2h(ctx, snapshots, d + off_snap, sizeof(c64) * (size_t)A * *n_iter));
  if (residual_rows) ISAC_TRY(copy_d2h(ctx, residual_rows, d_R, sizeof(c64) * n_rows_el));
  return ISAC_OK;
}
