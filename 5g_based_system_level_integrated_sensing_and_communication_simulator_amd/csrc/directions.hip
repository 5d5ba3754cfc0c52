// Off-grid direction finding with several sources per array snapshot (gfx950 only): isac_resolve_directions (include/isac_directions.h; project-defined).
// One array geometry serves both array types: element e = n + ny m at phase 2 pi d (m u + n v); the ULA is ny = 1, u = f / d, v = 0, one grid row, one maximiser round.
// directions_kernel: one workgroup of 256 threads per entry runs the greedy pass and every RELAX cycle in one launch; nothing goes through global memory in between.
//   thread e < A owns element e: x[e] and the residual r[e] live in its registers, the K directions and amplitudes in LDS (written by thread 0, read by all).
//   dir_eval     (S, D) = sum_e r[e] e^{+j phase} (1, w_e), w = m or n: one sincos of the full argument per thread, a butterfly sum inside each wave that holds elements
//                (x + y == y + x bit for bit, so all 64 lanes end with the same bits), one LDS word per wave, and EVERY thread adds the (at most 4) wave sums in ascending
//                order: all 256 threads hold the same bits and take the same branches, nothing is broadcast back.  The wave sums alternate between two LDS slots, so an
//                evaluation costs one barrier.
//   dir_axis     the 1-D maximiser of the header: both ends of the box, then kDirBisect halvings on the sign of dB/dt = -4 pi d Im(conj(S) D) -- 42 evaluations whatever the data.
//   coarse       the residual goes to LDS (s_r) and one lane per grid point forms B.  Direct form (the ULA, and planar arrays whose tables would not fit): A sincos per
//                point, r[e] one address for all lanes -- a broadcast.  Separable form (planar arrays with 16 (4 nx^2 + 4 ny^2 + 4 A) <= 96 KB, 48 KB at 16 x 16): per-axis
//                phasor tables E_u [nx][G_u], E_v [ny][G_v] formed once per workgroup, then per greedy step a row transform T[m][g_v] = sum_n r[n + ny m] E_v[n][g_v] and a
//                column transform S[g_u, g_v] = sum_m E_u[m][g_u] T[m][g_v].  Lanes run along g_v / g_u: consecutive 16-byte words (ds_read_b128 serves 16 lanes per cycle,
//                16 consecutive c64 cover each of the 64 banks once: conflict-free); the other operand is one address per lane group (broadcast).
//   arg-max      (value, lowest index): per thread the first maximum in ascending index order, a butterfly inside the wave, the 4 wave results joined by every thread.
// fp64 throughout, no atomics, no grid-wide sync: an entry's result is a function of its snapshot alone.  The order by power, n_src, the angles and the NaN fill are the
// host's (plain C++, one place).
#include <algorithm>
#include <cmath>
#include <vector>

#include "isac_internal.hpp"
#include "upa_steer.hpp"

namespace isac {

constexpr int kDirBisect = 40;                                            // the box 2 h = half a lobe shrinks by 2^-40: 4.5e-13 of a lobe, every entry the same count
constexpr int kDirRounds = 3;                                             // planar array: (u, then v) this many times
constexpr size_t kDirTableMax = 96 * 1024;                                // the separable coarse search where its tables fit this

struct DirGeom {
  int A, nx, ny, Gu, Gv;                                                  // elements, per axis; coarse grid points per axis (ULA: ny = 1, Gv = 1)
  int two_d;                                                              // planar array: the v axis exists, points outside the disc are left out, results are projected
  int tables;                                                             // separable coarse search
};

struct DirSD { c64 S, D; };

__device__ __forceinline__ double dir_phase(int m, int n, double u, double v) { return (2.0 * M_PI * kUpaSpacing) * ((double)m * u + (double)n * v); }
__device__ __forceinline__ c64 dir_phasor(double arg) {
  double s, c;
  sincos(arg, &s, &c);
  return mk(c, s);
}
__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// (S, D) of the residual r (this thread's element) at (u, v); D weighted by m (axis 0) or n (axis 1).  s_red: LDS [2][4][4] doubles; *slot alternates.
__device__ __forceinline__ DirSD dir_eval(const DirGeom& g, c64 r, int m, int n, double u, double v, int axis, double* s_red, int* slot) {
  const int tid = threadIdx.x, wave = tid >> 6, n_waves = (g.A + 63) >> 6;
  double* red = s_red + 16 * (*slot);
  *slot ^= 1;
  if (wave < n_waves) {                                                   // wave-uniform
    c64 z = mk(0.0, 0.0);
    if (tid < g.A) z = r * dir_phasor(dir_phase(m, n, u, v));
    const double w = (double)(axis ? n : m);
    const double a0 = wave_sum(z.re), a1 = wave_sum(z.im), a2 = wave_sum(w * z.re), a3 = wave_sum(w * z.im);
    if ((tid & 63) == 0) { red[4 * wave] = a0; red[4 * wave + 1] = a1; red[4 * wave + 2] = a2; red[4 * wave + 3] = a3; }
  }
  __syncthreads();
  DirSD o{mk(0.0, 0.0), mk(0.0, 0.0)};
  for (int w = 0; w < n_waves; ++w) { o.S.re += red[4 * w]; o.S.im += red[4 * w + 1]; o.D.re += red[4 * w + 2]; o.D.im += red[4 * w + 3]; }
  return o;
}

// the sign carrier of dB/dt on `axis` at t: -Im(conj(S) D)
__device__ __forceinline__ double dir_slope(const DirGeom& g, c64 r, int m, int n, double u, double v, int axis, double* s_red, int* slot) {
  const DirSD e = dir_eval(g, r, m, n, u, v, axis, s_red, slot);
  return e.S.im * e.D.re - e.S.re * e.D.im;
}

// the 1-D maximiser around centre c on `axis` (half width h), the other coordinate held at `other`
__device__ __forceinline__ double dir_axis(const DirGeom& g, c64 r, int m, int n, double c, double h, double other, int axis, double* s_red, int* slot) {
  auto slope = [&](double t) { return axis ? dir_slope(g, r, m, n, other, t, 1, s_red, slot) : dir_slope(g, r, m, n, t, other, 0, s_red, slot); };
  double lo = c - h, hi = c + h;
  const double g_lo = slope(lo), g_hi = slope(hi);
  const bool ok = g_lo > 0.0 && g_hi < 0.0;                                // NaN: false
  for (int it = 0; it < kDirBisect; ++it) {
    const double mid = 0.5 * (lo + hi);
    if (slope(mid) > 0.0) lo = mid; else hi = mid;
  }
  return ok ? 0.5 * (lo + hi) : c;
}

// the maximiser of B_r in the box of one coarse step around (u0, v0), projected (planar) or wrapped (linear); *u, *v on return
__device__ __forceinline__ void dir_maximise(const DirGeom& g, c64 r, int m, int n, double u0, double v0, double* u_out, double* v_out, double* s_red, int* slot) {
  const double hu = 2.0 / (double)g.Gu, hv = 2.0 / (double)g.Gv;
  double u = u0, v = v0;
  if (g.two_d) {
    for (int round = 0; round < kDirRounds; ++round) {
      u = dir_axis(g, r, m, n, u0, hu, v, 0, s_red, slot);
      v = dir_axis(g, r, m, n, v0, hv, u, 1, s_red, slot);
    }
    const double rad = hypot(u, v);
    if (rad > 1.0) { u = u / rad; v = v / rad; }
  } else {
    u = dir_axis(g, r, m, n, u0, hu, 0.0, 0, s_red, slot);
    if (u < -1.0) u += 2.0;                                               // period 2 in u = f / d: back into [-1, 1)
    if (u >= 1.0) u -= 2.0;
  }
  *u_out = u;
  *v_out = v;
}

__global__ __launch_bounds__(256) void directions_kernel(const c64* __restrict__ snap /* [A x n] */, DirGeom g, int K, int cycles, int* __restrict__ n_found_out /* [n] */,
                                                         double* __restrict__ u_out, double* __restrict__ v_out /* [K x n] */, c64* __restrict__ amp_out /* [K x n] */,
                                                         double* __restrict__ res_out /* [n] */) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  c64* s_r = reinterpret_cast<c64*>(smem_raw);                            // [A] the residual, for the coarse search
  c64* s_eu = s_r + g.A;                                                  // [nx][Gu]   (separable form only)
  c64* s_ev = s_eu + (g.tables ? g.nx * g.Gu : 0);                        // [ny][Gv]
  c64* s_t = s_ev + (g.tables ? g.ny * g.Gv : 0);                         // [nx][Gv]
  __shared__ double s_red[32];
  __shared__ double s_bv[4];
  __shared__ int s_bi[4];
  __shared__ double s_pu[ISAC_DIR_MAX_SOURCES], s_pv[ISAC_DIR_MAX_SOURCES];
  __shared__ c64 s_al[ISAC_DIR_MAX_SOURCES];
  const int tid = threadIdx.x, t = blockIdx.x, A = g.A;
  const int m = tid < A ? tid / g.ny : 0, n = tid < A ? tid % g.ny : 0;
  const c64 xx = tid < A ? snap[tid + (long long)A * t] : mk(0.0, 0.0);
  const double inv_a = 1.0 / (double)A;
  int slot = 0;
  auto grid_u = [&](int gu) { return -1.0 + (2.0 * (double)gu) / (double)g.Gu; };
  auto grid_v = [&](int gv) { return g.two_d ? -1.0 + (2.0 * (double)gv) / (double)g.Gv : 0.0; };
  // x minus every source in [0, count) but `skip`
  auto residual = [&](int count, int skip) {
    c64 r = xx;
    if (tid < A)
      for (int i = 0; i < count; ++i) {
        if (i == skip) continue;
        const c64 e = dir_phasor(dir_phase(m, n, s_pu[i], s_pv[i]));      // a_i[e] = conj(e)
        r = r - s_al[i] * conj(e);
      }
    return r;
  };
  if (g.tables) {
    for (int i = tid; i < g.nx * g.Gu; i += 256) s_eu[i] = dir_phasor(dir_phase(i / g.Gu, 0, grid_u(i % g.Gu), 0.0));
    for (int i = tid; i < g.ny * g.Gv; i += 256) s_ev[i] = dir_phasor(dir_phase(0, i / g.Gv, 0.0, grid_v(i % g.Gv)));
  }
  int found = 0;
  for (int k = 0; k < K; ++k) {
    const c64 rr = residual(k, -1);
    __syncthreads();                                                      // the previous pass is done with s_r / s_t; the tables are there
    if (tid < A) s_r[tid] = rr;
    __syncthreads();
    // ---- coarse search
    if (g.tables) {
      for (int i = tid; i < g.nx * g.Gv; i += 256) {
        const int mm = i / g.Gv, gv = i % g.Gv;
        c64 acc = mk(0.0, 0.0);
        for (int nn = 0; nn < g.ny; ++nn) acc = fma(s_r[nn + g.ny * mm], s_ev[nn * g.Gv + gv], acc);
        s_t[i] = acc;
      }
      __syncthreads();
    }
    double best = -1.0;                                                   // B >= 0; NaN never wins
    int best_i = 0x7fffffff;
    for (int i = tid; i < g.Gu * g.Gv; i += 256) {
      const int gu = i % g.Gu, gv = i / g.Gu;
      const double u = grid_u(gu), v = grid_v(gv);
      if (u * u + v * v > 1.0) continue;
      c64 acc = mk(0.0, 0.0);
      if (g.tables) {
        for (int mm = 0; mm < g.nx; ++mm) acc = fma(s_eu[mm * g.Gu + gu], s_t[mm * g.Gv + gv], acc);
      } else {
        for (int e = 0; e < A; ++e) acc = fma(s_r[e], dir_phasor(dir_phase(e / g.ny, e % g.ny, u, v)), acc);
      }
      const double b = acc.re * acc.re + acc.im * acc.im;
      if (b > best) { best = b; best_i = i; }
    }
    for (int o = 32; o > 0; o >>= 1) {
      const double v2 = __shfl_xor(best, o);
      const int i2 = __shfl_xor(best_i, o);
      if (v2 > best || (v2 == best && i2 < best_i)) { best = v2; best_i = i2; }
    }
    if ((tid & 63) == 0) { s_bv[tid >> 6] = best; s_bi[tid >> 6] = best_i; }
    __syncthreads();
    best = s_bv[0];
    best_i = s_bi[0];
    for (int w = 1; w < 4; ++w)
      if (s_bv[w] > best || (s_bv[w] == best && s_bi[w] < best_i)) { best = s_bv[w]; best_i = s_bi[w]; }
    if (!(best > 0.0)) break;                                             // no winner, or a maximum of 0: every thread alike
    // ---- maximiser and amplitude of source k
    double u, v;
    dir_maximise(g, rr, m, n, grid_u(best_i % g.Gu), grid_v(best_i / g.Gu), &u, &v, s_red, &slot);
    c64 al = dir_eval(g, rr, m, n, u, v, 0, s_red, &slot).S * inv_a;
    if (tid == 0) { s_pu[k] = u; s_pv[k] = v; s_al[k] = al; }
    __syncthreads();
    found = k + 1;
    // ---- RELAX
    if (k >= 1)
      for (int c = 0; c < cycles; ++c)
        for (int j = 0; j <= k; ++j) {
          const c64 rj = residual(k + 1, j);
          dir_maximise(g, rj, m, n, s_pu[j], s_pv[j], &u, &v, s_red, &slot);
          al = dir_eval(g, rj, m, n, u, v, 0, s_red, &slot).S * inv_a;   // (its barrier: every thread has read s_pu / s_pv / s_al)
          if (tid == 0) { s_pu[j] = u; s_pv[j] = v; s_al[j] = al; }
          __syncthreads();
        }
  }
  // ---- ||x - sum alpha a||^2 / A: the wave sums of |r|^2 through dir_eval's slots
  const c64 rf = residual(found, -1);
  double* red = s_red + 16 * slot;
  const double p = wave_sum(tid < A ? rf.re * rf.re + rf.im * rf.im : 0.0);
  if ((tid & 63) == 0) red[tid >> 6] = p;
  __syncthreads();
  if (tid == 0) {
    double sum = 0.0;
    for (int w = 0; w < 4; ++w) sum += red[w];
    res_out[t] = sum * inv_a;
    n_found_out[t] = found;
    for (int k = 0; k < found; ++k) {
      u_out[k + (long long)K * t] = s_pu[k];
      v_out[k + (long long)K * t] = s_pv[k];
      amp_out[k + (long long)K * t] = s_al[k];
    }
  }
}

}  // namespace isac

// ================================================================= host side
using namespace isac;

extern "C" int isac_resolve_directions(isac_ctx* ctx, const isac_est_params* ep, const isac_c64* snapshots, int32_t A, int32_t n, int32_t max_sources, int32_t cycles,
                                       double min_ratio, double min_power, int32_t* status, int32_t* n_found, int32_t* n_src, double* azi, double* ele, double* dir_u,
                                       double* dir_v, double* power, isac_c64* amp, double* residual) {
  ISAC_ENTER(ctx);
  const char* who = "isac_resolve_directions";
  if (!ep || !status || !n_found || !n_src || !azi || !dir_u || !power || n < 0 || n > ISAC_MAX_TARGETS || (n > 0 && !snapshots))
    return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": bad arguments");
  const bool upa = ep->array_is_upa != 0;
  if (upa && (!ele || !dir_v)) return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": a planar array needs ele and dir_v");
  if (A < 2) return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": at least two elements");
  if (upa && (ep->n_ants_x < 1 || ep->n_ants_y < 1 || (long long)ep->n_ants_x * ep->n_ants_y != A))
    return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": n_ants_x n_ants_y must equal A");
  if (max_sources < 1 || max_sources > ISAC_DIR_MAX_SOURCES || max_sources > A - 1)
    return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": max_sources must lie in 1 .. min(ISAC_DIR_MAX_SOURCES, A - 1)");
  if (cycles < 0 || !std::isfinite(min_ratio) || min_ratio < 0.0 || min_ratio > 1.0 || !std::isfinite(min_power) || min_power < 0.0)
    return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": cycles >= 0, min_ratio in [0, 1] and a finite min_power >= 0 are required");
  if (A > 256) return fail(ctx, ISAC_ERR_UNSUPPORTED, std::string(who) + ": more than 256 elements");
  if (n == 0) return ISAC_OK;
  DirGeom g{};
  g.A = A;
  g.nx = upa ? ep->n_ants_x : A;
  g.ny = upa ? ep->n_ants_y : 1;
  g.Gu = 4 * g.nx;
  g.Gv = upa ? 4 * g.ny : 1;
  g.two_d = upa ? 1 : 0;
  const size_t table_bytes = sizeof(c64) * ((size_t)g.nx * g.Gu + (size_t)g.ny * g.Gv + (size_t)g.nx * g.Gv);
  g.tables = upa && table_bytes <= kDirTableMax ? 1 : 0;
  const size_t lds = sizeof(c64) * (size_t)A + (g.tables ? table_bytes : 0);
  const int K = max_sources;
  // one scratch block: the snapshots [A x n] | amp [K x n] | u | v [K x n] | residual [n] | n_found [n]
  const size_t kn = (size_t)K * n, off_amp = sizeof(c64) * (size_t)A * n, off_u = off_amp + sizeof(c64) * kn, off_v = off_u + sizeof(double) * kn;
  const size_t off_res = off_v + sizeof(double) * kn, off_nf = off_res + sizeof(double) * (size_t)n;
  ISAC_TRY(ensure(ctx, ctx->directions, off_nf + sizeof(int) * (size_t)n));
  char* d = (char*)ctx->directions.p;
  ISAC_TRY(copy_h2d(ctx, d, snapshots, off_amp));
  ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(directions_kernel), lds));
  hipLaunchKernelGGL(directions_kernel, dim3(n), dim3(256), lds, ctx->stream, (const c64*)d, g, K, (int)cycles, (int*)(d + off_nf), (double*)(d + off_u), (double*)(d + off_v),
                     (c64*)(d + off_amp), (double*)(d + off_res));
  ISAC_HIP(hipGetLastError());
  std::vector<c64> h_amp(kn);
  std::vector<double> h_u(kn), h_v(kn), h_res((size_t)n);
  std::vector<int> h_nf((size_t)n);
  ISAC_TRY(copy_d2h(ctx, h_nf.data(), d + off_nf, sizeof(int) * (size_t)n));
  ISAC_TRY(copy_d2h(ctx, h_amp.data(), d + off_amp, sizeof(c64) * kn));
  ISAC_TRY(copy_d2h(ctx, h_u.data(), d + off_u, sizeof(double) * kn));
  ISAC_TRY(copy_d2h(ctx, h_v.data(), d + off_v, sizeof(double) * kn));
  ISAC_TRY(copy_d2h(ctx, h_res.data(), d + off_res, sizeof(double) * (size_t)n));
  // ---- step 2 and 3 of the header: order, floors, angles, fill
  const double deg = 180.0 / M_PI, nan = std::nan("");
  for (int i = 0; i < n; ++i) {
    const int nf = h_nf[(size_t)i];
    const size_t base = (size_t)K * i;
    int order[ISAC_DIR_MAX_SOURCES];
    double pw[ISAC_DIR_MAX_SOURCES];
    for (int k = 0; k < nf; ++k) {
      order[k] = k;
      pw[k] = h_amp[base + k].re * h_amp[base + k].re + h_amp[base + k].im * h_amp[base + k].im;
    }
    std::stable_sort(order, order + nf, [&](int a, int b) { return pw[a] > pw[b]; });
    int ns = 0;
    while (ns < nf && pw[order[ns]] >= min_ratio * pw[order[0]] && pw[order[ns]] >= min_power) ++ns;
    status[i] = nf == 0 ? 1 : 0;
    n_found[i] = nf;
    n_src[i] = ns;
    if (residual) residual[i] = h_res[(size_t)i];
    for (int k = 0; k < K; ++k) {
      const size_t o = base + k;
      if (k >= nf) {
        azi[o] = dir_u[o] = power[o] = nan;
        if (upa) ele[o] = dir_v[o] = nan;
        if (amp) amp[o] = isac_c64{0.0, 0.0};
        continue;
      }
      const size_t s = base + order[k];
      const double u = h_u[s], v = h_v[s];
      dir_u[o] = u;
      power[o] = pw[order[k]];
      if (amp) amp[o] = isac_c64{h_amp[s].re, h_amp[s].im};
      if (upa) {
        dir_v[o] = v;
        ele[o] = std::asin(std::fmin(1.0, std::hypot(u, v))) * deg;
        azi[o] = std::atan2(v, u) * deg;
      } else {
        azi[o] = std::asin(u) * deg;
      }
    }
  }
  return ISAC_OK;
}
