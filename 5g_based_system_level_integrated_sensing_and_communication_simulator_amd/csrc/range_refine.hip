// Off-grid range of listed targets from the two grids of a CPI (gfx950 only): isac_range_refine_dev (include/isac_subsample.h; project-defined).
// For entry i with rdm row r and Doppler frequency nu, H = rx .* conj(tx) [K x L x A], w = kaiser(K, 3):
//   c_i[k, a] = sum_l H[k, l, a] e^{-2 pi j nu l}                                        range_contract_kernel, a chunk of kRangeChunk entries per pass over the grids
//   Z_a(rho)  = nIFFT^{-1/2} sum_k w_k c_i[k, a] e^{+2 pi j k rho / nIFFT},  P = sum_a |Z_a|^2 / nFFT      range_search_kernel, one workgroup per entry
//   1  probes rho_g = (r - 1) + g / 8, g = -8 .. 8      2  the largest interior local maximum of P_g, lowest g on a tie; none: status 1
//   3  rho* = the zero of P' in [rho_{g-1}, rho_{g+1}] by kRangeBisect halvings on the sign of P'; power = P(rho*), snapshot Z(rho*) / sqrt(nFFT)
// range_contract_kernel is the hot path: a [K A x L] . [L x E] complex product whose left operand is formed on the fly.  One thread per (k, a), k fastest: for every l the
// lanes of a wave read 1 KB of each grid, contiguous, every value once; the E = kRangeChunk accumulators of a thread stay in registers and the phasors e^{-2 pi j nu_e l},
// the same for every lane, come from a table [L x E] through the scalar cache (a wave-uniform address), not from LDS: at E = 16 an LDS broadcast per (l, e) would cost
// more LDS cycles than the 4 fp64 FMAs it feeds cost the SIMD.  The sum over l runs ascending in one thread: no reduction, no atomics, and slot e's arithmetic does not
// depend on the other slots -- a chunk that is not full carries nu = 0 in its spare slots and their planes are never read.  Plain VALU fp64 rather than
// v_mfma_f64_16x16x4_f64: with E = 16 the pass asks for 8 E = 128 flops per 32 bytes read, a quarter of what the vector units deliver per HBM byte, so the kernel is bound
// by the two reads either way (DESIGN.md section 5 has the measurement), and the MFMA's [16 x 4] operand layout would want H transposed through LDS first.
// range_search_kernel: every evaluation of (P, P') at one rho forms its K phasors w_k e^{2 pi j k rho / nIFFT} anew in LDS (the turn count k rho / nIFFT reduced modulo 1
// before one sincospi; never a rotation by recurrence); wave v sums the antennas v, v + 4, ..: lane j the terms k = j, j + 64, .. ascending, joined by a butterfly of six
// xor shuffles (the same tree in every lane); the per-antenna terms |X_a|^2 and -Im(conj(X_a) D_a), D_a = sum_k k w_k c e^{..} (Z_a' = 2 pi j D_a / nIFFT^{3/2}), are left in
// LDS and summed by EVERY thread in ascending antenna order, as in refine_eval (refine_dev.hpp): all threads hold the same bits and take the same branch.
#include <cmath>
#include <vector>

#include "isac_internal.hpp"
#include "refine_dev.hpp"
#include "../../include/isac_subsample.h"

namespace isac {

constexpr int kRangeChunk = ISAC_RANGE_REFINE_CHUNK;                      // E: entries per pass over the grids
constexpr int kRangeBisect = 40;                                          // the bracket 1/4 bin shrinks by 2^-40: 2.3e-13 bin, every entry the same count
constexpr int kRangeProbes = 8;                                           // a side, 1/8 bin apart
static_assert(kRangeChunk == 16, "include/isac_subsample.h states the scratch bound for 16 entries");

// tab[l E + e] = e^{-2 pi j nu_e l}: sincos of the full argument (refine_phasor: the phasor isac_fft2d_refine_targets uses)
__global__ __launch_bounds__(256) void range_doppler_table_kernel(const double* __restrict__ nu /* [E] */, int L, c64* __restrict__ tab /* [L x E] */) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= L * kRangeChunk) return;
  tab[i] = refine_phasor(nu[i % kRangeChunk], i / kRangeChunk);
}

template <int E>
__global__ __launch_bounds__(256) void range_contract_kernel(const c64* __restrict__ rx, const c64* __restrict__ tx /* [K x L x A] */, int K, int L, int A,
                                                             const c64* __restrict__ tab /* [L x E] */, c64* __restrict__ c /* [E][A][K] */) {
  const long long KA = (long long)K * A;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;       // = k + K a
  if (idx >= KA) return;
  const long long a = idx / K, k = idx - a * K;
  const long long base = k + (long long)K * L * a;                       // element (k, 0, a); (k, l, a) is K l further
  c64 acc[E];
#pragma unroll
  for (int e = 0; e < E; ++e) acc[e] = mk(0.0, 0.0);
#pragma unroll 4
  for (int l = 0; l < L; ++l) {
    const c64 r = rx[base + (long long)K * l], t = tx[base + (long long)K * l];
    const c64 h = mul_conj(r, t);
    const c64* ph = tab + (long long)l * E;                              // wave-uniform: scalar loads
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = fma(h, ph[e], acc[e]);
  }
#pragma unroll
  for (int e = 0; e < E; ++e) c[(long long)e * KA + idx] = acc[e];
}

struct RangeSums { double p, d; };                                        // sum_a |X_a|^2, -sum_a Im(conj(X_a) D_a): P nFFT nIFFT and P' nFFT nIFFT^2 / 4 pi

// (p, d) at rho for the entry whose plane is ce [A][K]; on return every thread holds the same sums and s_x [A] = X_a(rho) = sqrt(nIFFT) Z_a(rho).  Ends with a barrier.
__device__ __forceinline__ RangeSums range_eval(const c64* __restrict__ ce, const double* __restrict__ win_k, int K, int A, double n_ifft, double rho, c64* s_ph, c64* s_x,
                                                double* s_p, double* s_d) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int k = tid; k < K; k += 256) {
    double t = ((double)k * rho) / n_ifft;                               // turns
    t -= rint(t);
    double s, co;
    sincospi(2.0 * t, &s, &co);
    const double w = win_k[k];
    s_ph[k] = mk(w * co, w * s);
  }
  __syncthreads();
  for (int a = wave; a < A; a += 4) {                                     // (wave-uniform)
    const c64* ca = ce + (long long)K * a;
    c64 x = mk(0.0, 0.0), dx = mk(0.0, 0.0);
    for (int k = lane; k < K; k += 64) {
      const c64 z = ca[k] * s_ph[k];
      x += z;
      dx = mk(::fma((double)k, z.re, dx.re), ::fma((double)k, z.im, dx.im));
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      x.re += __shfl_xor(x.re, m); x.im += __shfl_xor(x.im, m); dx.re += __shfl_xor(dx.re, m); dx.im += __shfl_xor(dx.im, m);
    }
    if (lane == 0) {
      s_x[a] = x;
      s_p[a] = x.re * x.re + x.im * x.im;
      s_d[a] = x.im * dx.re - x.re * dx.im;
    }
  }
  __syncthreads();
  RangeSums r{0.0, 0.0};
  for (int a = 0; a < A; ++a) { r.p += s_p[a]; r.d += s_d[a]; }           // ascending antenna order from 0.0; every lane the same address: broadcasts
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void range_search_kernel(const c64* __restrict__ c /* [E][A][K] */, const double* __restrict__ win_k, int K, int A, int n_ifft_i, int n_fft_i,
                                                           const int* __restrict__ row /* 1-based, this chunk's */, int probe_only, int* __restrict__ status,
                                                           double* __restrict__ rho_out, double* __restrict__ pow_out, c64* __restrict__ snap /* [A x chunk] */) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  c64* s_ph = reinterpret_cast<c64*>(smem_raw);                           // [K]
  c64* s_x = s_ph + K;                                                    // [A]
  double* s_p = reinterpret_cast<double*>(s_x + A);                       // [A]
  double* s_d = s_p + A;                                                  // [A]
  const int tid = threadIdx.x, t = blockIdx.x;
  const c64* ce = c + (long long)t * K * A;
  const double n_ifft = (double)n_ifft_i, scale = (double)n_ifft_i * (double)n_fft_i;
  const double rho0 = (double)(row[t] - 1);
  constexpr int M = kRangeProbes, G = 2 * M + 1;
  auto rho_of = [&](int gi) { return rho0 + (double)(gi - M) / (double)M; };
  // ---- steps 1-2: the largest interior local maximum, the lowest g on a tie (P_g > P_{g-1} and P_g >= P_{g+1}: NaN and an all-zero plane give none)
  int best_gi = -1;
  if (!probe_only) {
    double p_m2 = 0.0, p_m1 = 0.0, best = 0.0;
    for (int gi = 0; gi < G; ++gi) {
      const double p = range_eval(ce, win_k, K, A, n_ifft, rho_of(gi), s_ph, s_x, s_p, s_d).p / scale;
      if (gi >= 2 && p_m1 > p_m2 && p_m1 >= p && (best_gi < 0 || p_m1 > best)) { best = p_m1; best_gi = gi - 1; }
      p_m2 = p_m1;
      p_m1 = p;
    }
  }
  // ---- step 3 (status 1 or 2: rho = rho0)
  double rho = rho0;
  if (best_gi >= 0) {
    double lo = rho_of(best_gi - 1), hi = rho_of(best_gi + 1);
    for (int it = 0; it < kRangeBisect; ++it) {
      const double mid = 0.5 * (lo + hi);
      if (range_eval(ce, win_k, K, A, n_ifft, mid, s_ph, s_x, s_p, s_d).d > 0.0) lo = mid; else hi = mid;   // P' > 0: the maximum lies above mid
    }
    rho = 0.5 * (lo + hi);
  }
  const double p = range_eval(ce, win_k, K, A, n_ifft, rho, s_ph, s_x, s_p, s_d).p / scale;
  const double root = sqrt(scale);
  for (int a = tid; a < A; a += 256) snap[a + (long long)A * t] = mk(s_x[a].re / root, s_x[a].im / root);
  if (tid == 0) {
    status[t] = probe_only ? 2 : best_gi < 0 ? 1 : 0;
    rho_out[t] = rho;
    pow_out[t] = p;
  }
}

}  // namespace isac

// ================================================================= host side
using namespace isac;

extern "C" int isac_range_refine_dev(isac_ctx* ctx, const isac_est_params* ep, const isac_c64* d_rx_grid, const isac_c64* d_tx_grid, int32_t K, int32_t L, int32_t A,
                                     const int32_t* row, const double* nu, int32_t n, int32_t probe_only, int32_t* status, double* rho, double* rng, double* power,
                                     isac_c64* snapshots) {
  ISAC_ENTER(ctx);
  const char* who = "isac_range_refine_dev";
  if (!ep || !d_rx_grid || !d_tx_grid) return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": NULL ep or grid (a lazy echo grid: isac_echo_grid_materialize_dev first)");
  if (n < 0 || n > ISAC_MAX_TARGETS || (n > 0 && (!row || !nu || !status || !rho || !rng || !power))) return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": bad arguments");
  if (K <= 0 || L <= 0 || A <= 0 || K > ep->n_ifft || ep->n_fft <= 0) return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": K, L, A > 0, K <= n_ifft and n_fft > 0 are required");
  if (A > ISAC_RANGE_REFINE_MAX_ANTS) return fail(ctx, ISAC_ERR_CAPACITY, std::string(who) + ": more than 256 antennas");
  if (K > ISAC_RANGE_REFINE_MAX_K) return fail(ctx, ISAC_ERR_UNSUPPORTED, std::string(who) + ": the phasors of more than 8192 subcarriers do not fit the LDS");
  for (int i = 0; i < n; ++i) {
    if (row[i] < 1 || row[i] > ep->n_ifft) return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": a row outside 1 .. n_ifft");
    if (!std::isfinite(nu[i])) return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": a nu that is not finite");
  }
  if (n == 0) return ISAC_OK;
  constexpr int E = kRangeChunk;
  const double *win_k = nullptr, *win_r = nullptr;
  ISAC_TRY(isac_get_windows(ctx, K, ep->n_ifft, &win_k, &win_r));
  // one scratch block: the chunk's planes [E][A][K] and phasor table [L x E]; per chunk slot: nu, row; per entry: status, rho, power, snapshot [A]
  Carver cv;
  const size_t off_c = cv.take(sizeof(c64) * (size_t)E * A * K), off_tab = cv.take(sizeof(c64) * (size_t)L * E);
  const size_t off_nu = cv.take(sizeof(double) * E), off_row = cv.take(sizeof(int) * E);
  const size_t off_st = cv.take(sizeof(int) * (size_t)n), off_rho = cv.take(sizeof(double) * (size_t)n), off_pw = cv.take(sizeof(double) * (size_t)n);
  const size_t off_snap = cv.take(sizeof(c64) * (size_t)A * n);
  ISAC_TRY(ensure(ctx, ctx->range_refine, cv.total));
  char* d = (char*)ctx->range_refine.p;
  const size_t lds = sizeof(c64) * ((size_t)K + A) + sizeof(double) * 2 * (size_t)A;
  ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(range_search_kernel), lds));
  for (int i0 = 0; i0 < n; i0 += E) {
    const int m = std::min(E, n - i0);
    struct { double nu[E]; int row[E]; } slot{};                            // spare slots: nu = 0, never searched
    static_assert(sizeof(slot) == sizeof(double) * E + sizeof(int) * E, "nu and row are uploaded as one block");
    for (int e = 0; e < m; ++e) { slot.nu[e] = nu[i0 + e]; slot.row[e] = row[i0 + e]; }
    ISAC_TRY(stage_upload(ctx, d + off_nu, &slot, sizeof(slot)));
    hipLaunchKernelGGL(range_doppler_table_kernel, dim3(cdiv((long long)L * E, 256)), dim3(256), 0, ctx->stream, (const double*)(d + off_nu), L, (c64*)(d + off_tab));
    ISAC_TRY(profile_begin(ctx));                                          // isac_profile_enable(ctx, 1): the event pair brackets the contraction of the call's last chunk
    hipLaunchKernelGGL((range_contract_kernel<E>), dim3(cdiv((long long)K * A, 256)), dim3(256), 0, ctx->stream, (const c64*)d_rx_grid, (const c64*)d_tx_grid, K, L, A,
                       (const c64*)(d + off_tab), (c64*)(d + off_c));
    ISAC_TRY(profile_end(ctx));
    hipLaunchKernelGGL(range_search_kernel, dim3(m), dim3(256), lds, ctx->stream, (const c64*)(d + off_c), win_k, K, A, ep->n_ifft, ep->n_fft, (const int*)(d + off_row),
                       probe_only ? 1 : 0, (int*)(d + off_st) + i0, (double*)(d + off_rho) + i0, (double*)(d + off_pw) + i0, (c64*)(d + off_snap) + (size_t)A * i0);
    ISAC_HIP(hipGetLastError());
  }
  ISAC_TRY(copy_d2h(ctx, status, d + off_st, sizeof(int) * (size_t)n));
  ISAC_TRY(copy_d2h(ctx, rho, d + off_rho, sizeof(double) * (size_t)n));
  ISAC_TRY(copy_d2h(ctx, power, d + off_pw, sizeof(double) * (size_t)n));
  if (snapshots) ISAC_TRY(copy_d2h(ctx, snapshots, d + off_snap, sizeof(c64) * (size_t)A * n));
  for (int i = 0; i < n; ++i) rng[i] = rho[i] * ep->r_res;
  return ISAC_OK;
}
