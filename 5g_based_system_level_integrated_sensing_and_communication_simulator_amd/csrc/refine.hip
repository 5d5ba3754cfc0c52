// Refinement of listed cells of the last completed fft2D (gfx950 only): isac_fft2d_refine_targets (include/isac_refine.h; project-defined).  For entry i
// with range row r and Doppler bin k, on the L symbols y[l, a] of ymid [n_rows x L x A] in natural order (no half swap, no truncation):
//   X_a(nu) = sum_l y[l, a] e^{-2 pi j nu l},  P(nu) = sum_a |X_a(nu)|^2 / nFFT
//   1  probes nu_g = k / nFFT + g W / M, g = -M .. M          2  the largest interior local maximum of P_g, lowest g on a tie; none: status 1
//   3  nu* = the zero of P' in [nu_{g-1}, nu_{g+1}] by kRefineBisect halvings on the sign of P'; power = P(nu*), snapshot X(nu*) / sqrt(nFFT); azimuth (elevation): the
//      scan of the lists on the snapshot (targets.hip: target_scan_snapshots)
//   4  merge and 5 sidelobe flags on the host
// refine_kernel: one workgroup of 256 threads per entry runs steps 1-3 in one launch.  Every evaluation of (P, P') at one nu is refine_eval (refine_dev.hpp, shared with clean.hip): the thread map of
// target_snapshot -- four lanes per antenna, each a quarter of the symbols in ascending order, joined (q0 + q1) + (q2 + q3) -- with the phasors e^{-2 pi j nu l} read from
// LDS (every antenna's lanes of a quarter read the same word: broadcasts), the per-antenna terms |X_a|^2 and Im(conj(X_a) D_a), D_a = sum_l l y e^{..} (X_a' = -2 pi j D_a,
// so P' = (4 pi / nFFT) sum_a Im(conj(X_a) D_a)), left in LDS and summed by EVERY thread in ascending antenna order: all 256 threads hold the same (P, P') bits and take the
// same branch, nothing is broadcast back.  The probe phasors, (2M + 1) L sincos of the full argument, are formed once per workgroup; a bisection step forms its L phasors
// anew (never a rotation by recurrence).  The row, L A c64 at stride n_rows, is re-read from L2 at every evaluation and never staged: at the bench shape it is 229 KB and
// does not fit the LDS, and a second code path for the shapes where it would is not worth a call that is off the timed path.  fp64 throughout, no
// atomics, no grid-wide sync, no result that depends on arrival order.
#include <cmath>
#include <vector>

#include "isac_internal.hpp"
#include "refine_dev.hpp"

namespace isac {

constexpr int kRefineBisect = 40;                                         // the bracket 2 W / M shrinks by 2^-40: |nu - nu*| L <= 2.3e-13 where nFFT >= L, every entry the same count

__global__ __launch_bounds__(256) void refine_kernel(const c64* __restrict__ ymid /* [n_rows x L x A] */, int n_rows, int L, int A, int n_fft,
                                                     const int* __restrict__ cell_row /* window row, 0-based */, const int* __restrict__ cell_k /* col - nFFT/2 - 1 */,
                                                     double W, int M, int* __restrict__ status /* [n] */, double* __restrict__ nu_out /* [n] */,
                                                     double* __restrict__ pow_out /* [n] */, c64* __restrict__ snap /* [A x n] */) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int G = 2 * M + 1;
  c64* s_tab = reinterpret_cast<c64*>(smem_raw);                          // [G][L] probe phasors
  c64* s_ph = s_tab + (size_t)G * L;                                      // [L] phasors of a bisection step
  c64* s_x = s_ph + L;                                                    // [A]
  double* s_p = reinterpret_cast<double*>(s_x + A);                       // [A]
  double* s_d = s_p + A;                                                  // [A]
  const int tid = threadIdx.x, t = blockIdx.x;
  const c64* row = ymid + cell_row[t];
  const double nu0 = (double)cell_k[t] / (double)n_fft, nfft = (double)n_fft;
  auto nu_of = [&](int gi) { return nu0 + ((double)(gi - M) * W) / (double)M; };
  // ---- step 1
  for (int i = tid; i < G * L; i += 256) s_tab[i] = refine_phasor(nu_of(i / L), i % L);
  __syncthreads();
  // ---- step 2: the largest interior local maximum, the lowest g on a tie (P_g > P_{g-1} and P_g >= P_{g+1}: NaN and an all-zero row give none)
  double p_m2 = 0.0, p_m1 = 0.0, best = 0.0;
  int best_gi = -1;
  for (int gi = 0; gi < G; ++gi) {
    const double p = refine_eval(row, n_rows, L, A, s_tab + (size_t)gi * L, s_x, s_p, s_d).p / nfft;
    if (gi >= 2 && p_m1 > p_m2 && p_m1 >= p && (best_gi < 0 || p_m1 > best)) { best = p_m1; best_gi = gi - 1; }
    p_m2 = p_m1;
    p_m1 = p;
  }
  // ---- step 3 (status 1: lo = hi = nu0, and the loop leaves them there)
  double lo = nu0, hi = nu0;
  if (best_gi >= 0) { lo = nu_of(best_gi - 1); hi = nu_of(best_gi + 1); }
  for (int it = 0; it < kRefineBisect; ++it) {
    const double mid = 0.5 * (lo + hi);
    for (int l = tid; l < L; l += 256) s_ph[l] = refine_phasor(mid, l);
    __syncthreads();
    if (refine_eval(row, n_rows, L, A, s_ph, s_x, s_p, s_d).d > 0.0) lo = mid; else hi = mid;   // P' > 0: the maximum lies above mid
  }
  const double nu = 0.5 * (lo + hi);
  for (int l = tid; l < L; l += 256) s_ph[l] = refine_phasor(nu, l);
  __syncthreads();
  const double p = refine_eval(row, n_rows, L, A, s_ph, s_x, s_p, s_d).p / nfft;
  const double sqrt_nfft = sqrt(nfft);
  for (int a = tid; a < A; a += 256) snap[a + (long long)A * t] = mk(s_x[a].re / sqrt_nfft, s_x[a].im / sqrt_nfft);
  if (tid == 0) {
    status[t] = best_gi < 0 ? 1 : 0;
    nu_out[t] = nu;
    pow_out[t] = p;
  }
}

}  // namespace isac

// ================================================================= host side
using namespace isac;

namespace {

// D^2(delta): the squared Doppler response of an unwindowed L-symbol tone delta away, D(0) = 1
double dirichlet2(double delta, int L) {
  const double s = std::sin(M_PI * delta);
  if (s == 0.0) return 1.0;
  const double d = std::sin(M_PI * delta * L) / (L * s);
  return d * d;
}

// W = max(1/L, 1/nFFT), M = ceil(8 L W) probes a side, and their LDS
int refine_plan(isac_ctx* ctx, const char* who, RefinePlan* plan) {
  const int A = ctx->tgt.A, L = ctx->tgt.L, n_fft = ctx->tgt.ep.n_fft;
  const bool wide = n_fft >= L;
  plan->W = wide ? 1.0 / L : 1.0 / n_fft;
  plan->M = wide ? 8 : (8 * L + n_fft - 1) / n_fft;
  plan->lds = sizeof(c64) * ((size_t)(2 * plan->M + 2) * L + A) + sizeof(double) * 2 * (size_t)A;
  if (plan->lds > 160 * 1024) return fail(ctx, ISAC_ERR_UNSUPPORTED, std::string(who) + ": the probe phasors of this many symbols do not fit the LDS");
  return ISAC_OK;
}

}  // namespace

int tone_plan(isac_ctx* ctx, const char* who, RefinePlan* plan) {
  ISAC_TRY(refine_plan(ctx, who, plan));
  if (ctx->tgt.ep.array_is_upa) {                                          // n_ants_x n_ants_y != A: ISAC_ERR_INVALID_ARG; A > 256: ISAC_ERR_UNSUPPORTED -- before any work
    const double* d_tab = nullptr;
    int e_steps = 0, a_steps = 0;
    ISAC_TRY(isac_doa2d_grid(ctx, &ctx->tgt.ep, ctx->tgt.A, &d_tab, &e_steps, &a_steps));
  }
  return ISAC_OK;
}

int refine_enqueue(isac_ctx* ctx, const RefinePlan& plan, const c64* d_rows, const int* d_cell_row, const int* d_cell_k, int n, int* d_status, double* d_nu, double* d_pow,
                   c64* d_snap) {
  const Fft2dCpi& ts = ctx->tgt;
  ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(refine_kernel), plan.lds));
  hipLaunchKernelGGL(refine_kernel, dim3(n), dim3(256), plan.lds, ctx->stream, d_rows, ts.win.nr, ts.L, ts.A, ts.ep.n_fft, d_cell_row, d_cell_k, plan.W, plan.M, d_status, d_nu,
                     d_pow, d_snap);
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}

extern "C" int isac_fft2d_refine_targets(isac_ctx* ctx, const int32_t* row, const int32_t* col, int32_t n, double merge_tol, int32_t merge_rows, double sidelobe_margin,
                                         int32_t* n_kept, int32_t* status, int32_t* parent, int32_t* sidelobe_of, double* nu, double* vel, double* power, double* azi, double* ele,
                                         isac_c64* snapshots) {
  ISAC_ENTER(ctx);
  const char* who = "isac_fft2d_refine_targets";
  if (!n_kept || n < 0 || n > ISAC_MAX_TARGETS || (n > 0 && (!row || !col || !status || !parent || !sidelobe_of || !nu || !vel || !power || !azi)))
    return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": bad arguments");
  if (!std::isfinite(merge_tol) || merge_tol < 0.0 || !std::isfinite(sidelobe_margin) || sidelobe_margin < 0.0 || merge_rows < 0)
    return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": merge_tol, merge_rows and sidelobe_margin must be finite and not negative");
  ISAC_TRY(cpi_ready(ctx, who));
  const Fft2dCpi& ts = ctx->tgt;
  const isac_est_params& ep = ts.ep;
  const CutWindow& w = ts.win;
  const int A = ts.A, L = ts.L, n_fft = ep.n_fft;
  if (ep.array_is_upa && n > 0 && !ele) return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": a planar array needs ele");
  *n_kept = 0;
  if (n == 0) return ISAC_OK;
  std::vector<int> sel((size_t)2 * n);                                    // [window row, 0-based | k]
  for (int i = 0; i < n; ++i) {
    if (row[i] < w.row0 || row[i] >= w.row0 + w.n_cut_rows || col[i] < w.col0 || col[i] >= w.col0 + w.n_cut_cols)
      return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": a cell outside the CUT zone of the CPI");
    sel[(size_t)i] = row[i] - w.first_row;
    sel[(size_t)n + i] = col[i] - n_fft / 2 - 1;
  }
  RefinePlan plan;
  ISAC_TRY(refine_plan(ctx, who, &plan));
  // one scratch block: [row | k], status, scan bin: ints; nu, power: doubles; the snapshots [A x n]
  Carver cv;
  const size_t off_sel = cv.take(sizeof(int) * 2 * (size_t)n), off_st = cv.take(sizeof(int) * (size_t)n), off_bin = cv.take(sizeof(int) * (size_t)n);
  const size_t off_nu = cv.take(sizeof(double) * (size_t)n), off_pw = cv.take(sizeof(double) * (size_t)n), off_snap = cv.take(sizeof(c64) * (size_t)A * n);
  ISAC_TRY(ensure(ctx, ctx->refine, cv.total));
  char* d = (char*)ctx->refine.p;
  ISAC_TRY(stage_upload(ctx, d + off_sel, sel.data(), sizeof(int) * sel.size()));
  ISAC_TRY(refine_enqueue(ctx, plan, (const c64*)ctx->ymid.p, (const int*)(d + off_sel), (const int*)(d + off_sel) + n, n, (int*)(d + off_st), (double*)(d + off_nu),
                          (double*)(d + off_pw), (c64*)(d + off_snap)));
  ISAC_TRY(target_scan_snapshots(ctx, (const c64*)(d + off_snap), n, (int*)(d + off_bin), azi, ele));
  ISAC_TRY(copy_d2h(ctx, status, d + off_st, sizeof(int) * (size_t)n));
  ISAC_TRY(copy_d2h(ctx, nu, d + off_nu, sizeof(double) * (size_t)n));
  ISAC_TRY(copy_d2h(ctx, power, d + off_pw, sizeof(double) * (size_t)n));
  if (snapshots) ISAC_TRY(copy_d2h(ctx, snapshots, d + off_snap, sizeof(c64) * (size_t)A * n));
  for (int i = 0; i < n; ++i) vel[i] = status[i] == 0 ? nu[i] * n_fft * ep.v_res : CutWindow::velocity_of(col[i], ep);
  // ---- step 4: in input order, the first earlier kept entry with status 0 within merge_rows rows and merge_tol / L of nu absorbs (merge_parent, cpi_post.hpp)
  for (int i = 0; i < n; ++i) {
    parent[i] = status[i] != 0 ? i : merge_parent(i, row, nu, parent, status, merge_rows, merge_tol, L);
    sidelobe_of[i] = -1;
  }
  // ---- step 5: a kept entry that a stronger kept entry's Doppler response explains is flagged
  int kept = 0;
  for (int i = 0; i < n; ++i) {
    if (parent[i] != i) continue;
    ++kept;
    if (status[i] != 0 || sidelobe_margin == 0.0) continue;
    for (int k = 0; k < n; ++k)
      if (k != i && parent[k] == k && status[k] == 0 && std::abs(row[i] - row[k]) <= merge_rows && power[k] > power[i] &&
          power[i] <= sidelobe_margin * power[k] * dirichlet2(nu[i] - nu[k], L)) { sidelobe_of[i] = k; break; }
  }
  *n_kept = kept;
  return ISAC_OK;
}
