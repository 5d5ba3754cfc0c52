// Joint re-fit (RELAX) of Doppler tones on the range rows of the last completed fft2D (gfx950 only): isac_fft2d_relax_targets (include/isac_relax.h; project-defined,
// DESIGN.md section 5).  On a copy R of the range rows ymid [nr x L x A], with C_j [span x A] the amplitudes of tone j on the rows of its span:
//   0  in input order: fit tone i at nu_in[i] on its span and subtract it (step 8 of isac_clean.h)
//   1  `cycles` times, in input order: (a, b) relax_nu_kernel: the zero of P' of the centre row with tone j restored, inside nu_j +- box / L; (c) relax_refit_kernel: on every
//      row of the span, restore tone j at its old frequency, fit it at the new one, subtract it -- one read-modify-write of the row
//   2  relax_out_kernel: power and snapshot from C_j on the centre row; direction: target_scan_snapshots (targets.hip)
// Step 0 IS relax_refit_kernel with C = 0 and old = new frequency: y + 0 conj(p) = y, so the fit and the subtraction are clean_cancel_kernel's -- both are
// tone_fit_subtract (refine_dev.hpp), which differs between them only as refine_eval<AddBack> does.  Both kernels evaluate through refine_eval<true> (refine_dev.hpp): the thread map and the order of summation of refine_kernel, the sample being y + C conj(p_old) formed
// on the fly.  relax_nu_kernel: one workgroup of 256 threads per entry, reads only, writes nu_new (and keeps nu_old beside it for the re-fit).  relax_refit_kernel: one
// workgroup per row of the span, as clean_cancel_kernel is laid out; a workgroup owns its row and its C_j row.
// Entries whose spans overlap (transitively) form a cluster; clusters share no row.  blockIdx.y runs over the clusters and one launch pair handles the k-th entry (input
// order) of every cluster: every row sees its entries in input order, so the result is that of the sequential sweep, bit for bit.  Nothing is read back until the end; no
// cooperative launch, no cross-workgroup synchronisation, no atomics, no loop bound that depends on the data.  fp64 throughout.
#include <cmath>
#include <cstring>
#include <vector>

#include "isac_internal.hpp"
#include "refine_dev.hpp"

namespace isac {

constexpr int kRelaxBisect = 40;                                          // halvings of the bracket 2 box / L: every entry, every cycle the same count

struct RelaxLds {                                                         // the dynamic LDS of both kernels
  c64 *back, *ph, *x;                                                     // [L] phasors of the old frequency, [L] of the one evaluated, [A] X_a
  double *p, *d;                                                          // [A] each
  __device__ RelaxLds(char* raw, int L, int A) : back(reinterpret_cast<c64*>(raw)), ph(back + L), x(ph + L), p(reinterpret_cast<double*>(x + A)), d(p + A) {}
  static size_t bytes(int L, int A) { return sizeof(c64) * (2 * (size_t)L + A) + sizeof(double) * 2 * (size_t)A; }
};

// sched [n_clusters x max_len]: the entries of cluster blockIdx.y in input order, -1 behind the last
__global__ __launch_bounds__(256) void relax_nu_kernel(const c64* __restrict__ R /* [nr x L x A] */, int nr, int L, int A, int S, const int* __restrict__ sched, int max_len, int k,
                                                       const int* __restrict__ wr /* centre window row, 0-based */, const int* __restrict__ lo /* first window row of the span */,
                                                       const c64* __restrict__ C /* [n x S x A] */, const unsigned char* __restrict__ active /* [L] */, double h,
                                                       double* nu /* [n] */, double* nu_prev /* [n] */, int* __restrict__ flag /* [n] */) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const RelaxLds s(smem_raw, L, A);
  const int j = sched[blockIdx.y * max_len + k];
  if (j < 0) return;                                                      // (the whole workgroup)
  const int tid = threadIdx.x;
  const c64* row = R + wr[j];
  const c64* c_row = C + ((size_t)j * S + (wr[j] - lo[j])) * A;
  const double nu_j = nu[j];
  auto dp_at = [&](double v) {                                            // the sign carrier of P_j'(v)
    tone_phasors(s.ph, v, L, active);
    __syncthreads();
    return refine_eval<true>(row, nr, L, A, s.ph, s.x, s.p, s.d, s.back, c_row).d;
  };
  tone_phasors(s.back, nu_j, L, active);                                 // (the barrier of the first dp_at covers it)
  const double d_lo = dp_at(nu_j - h), d_hi = dp_at(nu_j + h);
  const bool ok = d_lo > 0.0 && d_hi < 0.0;                               // NaN and an all-zero row: never
  double a = nu_j, b = nu_j;                                              // no bracket: the loop leaves them there
  if (ok) { a = nu_j - h; b = nu_j + h; }
  for (int it = 0; it < kRelaxBisect; ++it) {
    const double mid = 0.5 * (a + b);
    if (dp_at(mid) > 0.0) a = mid; else b = mid;                          // P' > 0: the maximum lies above mid
  }
  if (tid == 0) {                                                         // (every thread read nu[j] before the first barrier)
    nu_prev[j] = nu_j;
    nu[j] = 0.5 * (a + b);
    flag[j] = ok ? 0 : 1;
  }
}

__global__ __launch_bounds__(256) void relax_refit_kernel(c64* R /* [nr x L x A] */, int nr, int L, int A, int S, const int* __restrict__ sched, int max_len, int k,
                                                          const int* __restrict__ lo, const int* __restrict__ len /* rows of the span */, c64* C /* [n x S x A] */,
                                                          const unsigned char* __restrict__ active, double n_active, const double* __restrict__ nu,
                                                          const double* __restrict__ nu_prev) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const RelaxLds s(smem_raw, L, A);
  const int j = sched[blockIdx.y * max_len + k];
  if (j < 0 || (int)blockIdx.x >= len[j]) return;                         // (the whole workgroup)
  const int tid = threadIdx.x;
  c64* row = R + lo[j] + blockIdx.x;                                      // (the host clips the span to 0 .. nr - 1)
  c64* c_row = C + ((size_t)j * S + blockIdx.x) * A;
  tone_phasors(s.back, nu_prev[j], L, active);
  tone_phasors(s.ph, nu[j], L, active);
  __syncthreads();
  tone_fit_subtract<true>(row, nr, L, A, active, n_active, s.ph, s.x, s.p, s.d, s.back, c_row);   // s.x[a] = sum over the active symbols of (y + C conj(p_old)) p_new
  __syncthreads();                                                        // every read of the old C_j row is done
  for (int a = tid; a < A; a += 256) c_row[a] = mk(s.x[a].re / n_active, s.x[a].im / n_active);
}

// power[j] = sum_a |n_active C_j[row_j, a]|^2 / nFFT (ascending a from 0.0), snap[:, j] = n_active C_j[row_j, :] / sqrt(nFFT)
__global__ __launch_bounds__(256) void relax_out_kernel(const c64* __restrict__ C, int A, int S, const int* __restrict__ wr, const int* __restrict__ lo, double n_active, double nfft,
                                                        c64* __restrict__ snap /* [A x n] */, double* __restrict__ power /* [n] */) {
  const int j = blockIdx.x;
  const c64* c_row = C + ((size_t)j * S + (wr[j] - lo[j])) * A;
  const double sqrt_nfft = sqrt(nfft);
  for (int a = threadIdx.x; a < A; a += 256) snap[a + (long long)A * j] = mk((n_active * c_row[a].re) / sqrt_nfft, (n_active * c_row[a].im) / sqrt_nfft);
  if (threadIdx.x == 0) {
    double p = 0.0;
    for (int a = 0; a < A; ++a) {
      const double re = n_active * c_row[a].re, im = n_active * c_row[a].im;
      p += re * re + im * im;
    }
    power[j] = p / nfft;
  }
}

}  // namespace isac

// ================================================================= host side
using namespace isac;

extern "C" int isac_fft2d_relax_targets(isac_ctx* ctx, const int32_t* row, const double* nu_in, int32_t n, int32_t cycles, int32_t span_rows, double box, const uint8_t* sym_active,
                                        int32_t* status, double* nu, double* vel, double* power, double* shift, double* last_step, double* azi, double* ele, isac_c64* snapshots,
                                        isac_c64* residual_rows) {
  ISAC_ENTER(ctx);
  const char* who = "isac_fft2d_relax_targets";
  if (n < 0 || n > ISAC_RELAX_MAX_TONES || (n > 0 && (!row || !nu_in || !status || !nu || !vel || !power || !shift || !last_step || !azi)))
    return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": n must lie in 0..ISAC_RELAX_MAX_TONES and no required array may be NULL");
  if (cycles < 0 || cycles > 64 || span_rows < 0 || !std::isfinite(box) || box <= 0.0 || box > 2.0)
    return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": cycles must lie in 0..64, span_rows must not be negative, box must lie in (0, 2]");
  for (int i = 0; i < n; ++i)
    if (!std::isfinite(nu_in[i])) return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": a frequency that is not finite");
  ISAC_TRY(cpi_ready(ctx, who));
  const Fft2dCpi& ts = ctx->tgt;
  const isac_est_params& ep = ts.ep;
  const CutWindow& w = ts.win;
  const int A = ts.A, L = ts.L, n_fft = ep.n_fft;
  if (ep.array_is_upa && n > 0 && !ele) return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": a planar array needs ele");
  for (int i = 0; i < n; ++i)
    if (row[i] < w.row0 || row[i] >= w.row0 + w.n_cut_rows) return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": a row outside the CUT zone of the CPI");
  SymbolMask mask;
  ISAC_TRY(symbol_mask(ctx, who, sym_active, L, &mask));
  const int n_active = mask.n_active;
  const size_t n_rows_el = (size_t)w.nr * L * A;
  if (n == 0) {                                                            // nothing to fit: R is the copy of the range rows
    if (residual_rows) ISAC_TRY(copy_d2h(ctx, residual_rows, ctx->ymid.p, sizeof(c64) * n_rows_el));
    return ISAC_OK;
  }
  RefinePlan plan;
  ISAC_TRY(tone_plan(ctx, who, &plan));                                    // the LDS refusal of the refinement; both kernels here need less (2 L + A values against (2 M + 2) L + A, M >= 8)
  // ---- spans and clusters: entries whose spans share a row, transitively; the k-th entry (input order) of every cluster goes into launch pair k
  std::vector<int> wr((size_t)n), lo((size_t)n), len((size_t)n), cl((size_t)n);
  int S = 1;
  for (int i = 0; i < n; ++i) {
    wr[(size_t)i] = row[i] - w.first_row;                                  // 0 <= wr < nr: a CUT row of the window
    const RowSpan sp = span_of(wr[(size_t)i], span_rows, w.nr);
    lo[(size_t)i] = sp.lo;
    len[(size_t)i] = sp.len();
    S = std::max(S, len[(size_t)i]);
    cl[(size_t)i] = i;
  }
  for (bool moved = true; moved;) {                                        // label = the smallest index of the cluster (n <= 64)
    moved = false;
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < n; ++k)
        if (lo[(size_t)i] < lo[(size_t)k] + len[(size_t)k] && lo[(size_t)k] < lo[(size_t)i] + len[(size_t)i] && cl[(size_t)k] < cl[(size_t)i]) { cl[(size_t)i] = cl[(size_t)k]; moved = true; }
  }
  std::vector<std::vector<int>> members;
  std::vector<int> slot((size_t)n, -1);
  for (int i = 0; i < n; ++i) {
    const int c = cl[(size_t)i];
    if (slot[(size_t)c] < 0) { slot[(size_t)c] = (int)members.size(); members.emplace_back(); }
    members[(size_t)slot[(size_t)c]].push_back(i);
  }
  const int n_cl = (int)members.size();
  int max_len = 0;
  for (const auto& m : members) max_len = std::max(max_len, (int)m.size());
  std::vector<int> sched((size_t)n_cl * max_len, -1);
  for (int c = 0; c < n_cl; ++c)
    for (size_t k = 0; k < members[(size_t)c].size(); ++k) sched[(size_t)c * max_len + k] = members[(size_t)c][k];
  // ---- one scratch block: [R nr L A | C n S A | snapshots A n] c64, [nu | nu_prev | power] doubles, [wr | lo | len | flag | scan bin | sched] ints, the symbol mask [L]
  Carver cv;
  const size_t off_r = cv.take(sizeof(c64) * n_rows_el), off_c = cv.take(sizeof(c64) * (size_t)n * S * A), off_snap = cv.take(sizeof(c64) * (size_t)A * n);
  const size_t off_nu = cv.take(sizeof(double) * 3 * (size_t)n), off_int = cv.take(sizeof(int) * (5 * (size_t)n + sched.size())), off_act = cv.take((size_t)L);
  ISAC_TRY(ensure(ctx, ctx->relax, cv.total));
  char* d = (char*)ctx->relax.p;
  c64 *d_R = (c64*)(d + off_r), *d_C = (c64*)(d + off_c), *d_snap = (c64*)(d + off_snap);
  double *d_nu = (double*)(d + off_nu), *d_prev = d_nu + n, *d_pow = d_prev + n;
  int *d_wr = (int*)(d + off_int), *d_lo = d_wr + n, *d_len = d_lo + n, *d_flag = d_len + n, *d_bin = d_flag + n, *d_sched = d_bin + n;
  const unsigned char* d_act = (const unsigned char*)(d + off_act);
  std::vector<char> meta(cv.total - off_nu, 0);                            // everything behind the snapshots in one upload (power, flag and scan bin start as zeros)
  std::memcpy(meta.data(), nu_in, sizeof(double) * (size_t)n);
  std::memcpy(meta.data() + sizeof(double) * (size_t)n, nu_in, sizeof(double) * (size_t)n);
  int* m_int = (int*)(meta.data() + (off_int - off_nu));
  std::memcpy(m_int, wr.data(), sizeof(int) * (size_t)n);
  std::memcpy(m_int + n, lo.data(), sizeof(int) * (size_t)n);
  std::memcpy(m_int + 2 * (size_t)n, len.data(), sizeof(int) * (size_t)n);
  std::memcpy(m_int + 5 * (size_t)n, sched.data(), sizeof(int) * sched.size());
  std::memcpy(meta.data() + (off_act - off_nu), mask.act.data(), (size_t)L);
  ISAC_HIP(hipMemcpyAsync(d_R, ctx->ymid.p, sizeof(c64) * n_rows_el, hipMemcpyDeviceToDevice, ctx->stream));
  ISAC_HIP(hipMemsetAsync(d_C, 0, sizeof(c64) * (size_t)n * S * A, ctx->stream));
  ISAC_TRY(copy_h2d(ctx, d + off_nu, meta.data(), meta.size()));
  const size_t lds = RelaxLds::bytes(L, A);                                // (<= the refinement's, which tone_plan has bounded by 160 KB)
  ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(relax_nu_kernel), lds));
  ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(relax_refit_kernel), lds));
  const double h = box / (double)L;
  for (int cyc = 0; cyc <= cycles; ++cyc)                                  // cycle 0: step 0 (C = 0, nu_prev = nu = nu_in)
    for (int k = 0; k < max_len; ++k) {
      if (cyc > 0) {
        hipLaunchKernelGGL(relax_nu_kernel, dim3(1, n_cl), dim3(256), lds, ctx->stream, (const c64*)d_R, w.nr, L, A, S, (const int*)d_sched, max_len, k, (const int*)d_wr,
                           (const int*)d_lo, (const c64*)d_C, d_act, h, d_nu, d_prev, d_flag);
        ISAC_HIP(hipGetLastError());
      }
      hipLaunchKernelGGL(relax_refit_kernel, dim3(S, n_cl), dim3(256), lds, ctx->stream, d_R, w.nr, L, A, S, (const int*)d_sched, max_len, k, (const int*)d_lo, (const int*)d_len,
                         d_C, d_act, (double)n_active, (const double*)d_nu, (const double*)d_prev);
      ISAC_HIP(hipGetLastError());
    }
  hipLaunchKernelGGL(relax_out_kernel, dim3(n), dim3(256), 0, ctx->stream, (const c64*)d_C, A, S, (const int*)d_wr, (const int*)d_lo, (double)n_active, (double)n_fft, d_snap, d_pow);
  ISAC_HIP(hipGetLastError());
  ISAC_TRY(target_scan_snapshots(ctx, d_snap, n, d_bin, azi, ele));
  std::vector<double> prev((size_t)n);
  ISAC_TRY(copy_d2h(ctx, nu, d_nu, sizeof(double) * (size_t)n));
  ISAC_TRY(copy_d2h(ctx, prev.data(), d_prev, sizeof(double) * (size_t)n));
  ISAC_TRY(copy_d2h(ctx, power, d_pow, sizeof(double) * (size_t)n));
  ISAC_TRY(copy_d2h(ctx, status, d_flag, sizeof(int) * (size_t)n));
  if (snapshots) ISAC_TRY(copy_d2h(ctx, snapshots, d_snap, sizeof(c64) * (size_t)A * n));
  if (residual_rows) ISAC_TRY(copy_d2h(ctx, residual_rows, d_R, sizeof(c64) * n_rows_el));
  for (int i = 0; i < n; ++i) {
    vel[i] = nu[i] * n_fft * ep.v_res;
    shift[i] = std::fabs(nu[i] - nu_in[i]) * L;
    last_step[i] = std::fabs(nu[i] - prev[(size_t)i]) * L;               // cycles == 0: nu_prev = nu = nu_in
  }
  return ISAC_OK;
}
