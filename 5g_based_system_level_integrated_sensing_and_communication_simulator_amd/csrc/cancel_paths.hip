// Reference-signal cancellation on the received waveform (gfx950): isac_cancel_paths_dev (include/isac_cancel_paths.h).
//
//   R [M x T]   the reference columns: isac_path_coefs_on (multistatic.hip) with unit gains and one receive element -> ctx->coef, row m contiguous in t
//   G = R^H R, B = R^H Y, power_in = diag(Y^H Y)      ref_gram_kernel (one pass over R and Y, fp64 MFMA) + ref_reduce_kernel (fixed order)
//   C = G^-1 B                                        ref_solve_kernel (one workgroup: Cholesky in LDS, the dependence test, two triangular solves per element)
//   Y' = Y - R C, power_out = diag(Y'^H Y')           ref_subtract_kernel (one read of Y, one write; skipped by the record's flag) + ref_finish_kernel (fixed order)
// Y is column-major: an element's column is contiguous in t like a row of R, so both operands of R^H [R | Y] stream along t and the MFMA's k index is only a summation
// label (cov.hip's observation).  Only the M reference rows of the product of the stacked operand are formed -- isac_covariance_dev would form the A x A block as well.
// Nothing is accumulated with atomics: per-workgroup partials, reduced in a fixed order; the call gives the same bits every time, in place or out of place.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "isac_internal.hpp"

namespace isac {

typedef double v4f64 __attribute__((ext_vector_type(4)));

constexpr int kRefLd = 32;                 // leading dimension of G, B and C: ISAC_CANCEL_PATHS_MAX_REFS
static_assert(kRefLd == ISAC_CANCEL_PATHS_MAX_REFS, "G [32 x 32] is the solve kernel's LDS image");
constexpr int kSubCols = 16;               // receive elements per workgroup of ref_subtract_kernel
constexpr double kDependentPivot = 1e-10;  // include/isac_cancel_paths.h: a pivot <= 1e-10 G_mm

// What the call reads back: the header, then coef [M x A] and power [2 x A] (written by ref_finish_kernel on success only)
struct RefRecord { int dependent; int pad[3]; };
static_assert(sizeof(RefRecord) == 16, "coef behind the header is 16-byte aligned");

// ---------------------------------------------------------------- 1. G | B partials
// Grid (chunk of slabs, group of four column tiles): wave w of a workgroup owns column tile ct = 4 blockIdx.y + w of the stacked operand [R | Y] (tiles 0 .. NRT - 1: the
// references, padded to 16 NRT; then the elements of Y, 16 per tile) and forms its NRT row tiles over the chunk's slabs of 16 samples.  Lane (i = lane & 15, kq = lane >> 4)
// holds samples 16 s + 4 kq + e, e = 0 .. 3, of row 16 I + i of R and of column i of its tile: four 16-byte loads of 64 contiguous bytes each, at a clamped sample; what lies
// beyond T, M or A is replaced by zero when the slab is consumed.  Per sample three real MFMAs per row tile (the 3M form of cov_3m_kstep, cov.hip):
//   S1 += Rr Xr,  S2 += Ri Xi,  S3 += (Rr - Ri)(Xr + Xi)   =>   Re(R^H X) = S1 + S2,  Im(R^H X) = (S3 - S1) + S2
// issued in three sweeps over the row tiles and into two accumulator sets by the parity of e, so that two v_mfma_f64_16x16x4_f64 into the same accumulator are at least six
// issues apart at NRT = 1 (a dependent one waits for its predecessor's pass).  The next slab's loads are issued before the current slab's MFMAs.
// power_in: each lane of a Y tile sums |Y|^2 of its samples; ref_reduce_kernel adds the four kq lanes of an element over the chunks.
template <int NRT>
__global__ __launch_bounds__(256) void ref_gram_kernel(const c64* __restrict__ R, const c64* __restrict__ Y, long long T, int M, int A, long long slabs_per_wg, int n_ct,
                                                       double* __restrict__ part /* [chunks][NRT][n_ct][2][256] */, double* __restrict__ ppow /* [chunks][n_ct - NRT][64] */) {
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ct = blockIdx.y * 4 + wid;
  if (ct >= n_ct) return;                                                  // (no barrier in this kernel)
  const int li = lane & 15, kq = lane >> 4;
  const bool is_y = ct >= NRT;
  const c64* rowp[NRT];
  bool rowok[NRT];
#pragma unroll
  for (int I = 0; I < NRT; ++I) {
    const int m = 16 * I + li;
    rowok[I] = m < M;
    rowp[I] = R + (long long)(rowok[I] ? m : 0) * T;
  }
  const int c = (is_y ? 16 * (ct - NRT) : 16 * ct) + li;
  const bool colok = c < (is_y ? A : M);
  const c64* colp = (is_y ? Y : R) + (long long)(colok ? c : 0) * T;
  const long long total = (T + 15) / 16;
  const long long s_begin = (long long)blockIdx.x * slabs_per_wg;
  const long long s_end = std::min(total, s_begin + slabs_per_wg);
  v4f64 acc[2][NRT][3];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int I = 0; I < NRT; ++I)
#pragma unroll
      for (int k = 0; k < 3; ++k) acc[p][I][k] = v4f64{0.0, 0.0, 0.0, 0.0};
  double pw = 0.0;
  auto load = [&](c64 (&a)[NRT][4], c64 (&b)[4], long long s) {
    const long long t0 = s * 16 + 4 * kq;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long long tc = t0 + e < T ? t0 + e : T - 1;                    // unconditional loads at a clamped sample
#pragma unroll
      for (int I = 0; I < NRT; ++I) a[I][e] = rowp[I][tc];
      b[e] = colp[tc];
    }
  };
  auto consume = [&](const c64 (&a)[NRT][4], const c64 (&b)[4], long long s) {
    const long long t0 = s * 16 + 4 * kq;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool ok = t0 + e < T;
      const c64 bv = (ok && colok) ? b[e] : mk(0.0, 0.0);
      c64 av[NRT];
#pragma unroll
      for (int I = 0; I < NRT; ++I) av[I] = (ok && rowok[I]) ? a[I][e] : mk(0.0, 0.0);
      pw += bv.re * bv.re + bv.im * bv.im;
      const double bs = bv.re + bv.im;
#pragma unroll
      for (int I = 0; I < NRT; ++I) acc[e & 1][I][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[I].re, bv.re, acc[e & 1][I][0], 0, 0, 0);
#pragma unroll
      for (int I = 0; I < NRT; ++I) acc[e & 1][I][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[I].im, bv.im, acc[e & 1][I][1], 0, 0, 0);
#pragma unroll
      for (int I = 0; I < NRT; ++I) acc[e & 1][I][2] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[I].re - av[I].im, bs, acc[e & 1][I][2], 0, 0, 0);
    }
  };
  c64 a0[NRT][4], b0[4], a1[NRT][4], b1[4];
  if (s_begin < s_end) load(a0, b0, s_begin);
  for (long long s = s_begin; s < s_end; s += 2) {                         // two register sets in rotation
    load(a1, b1, s + 1 < s_end ? s + 1 : s);
    consume(a0, b0, s);
    if (s + 1 >= s_end) break;
    load(a0, b0, s + 2 < s_end ? s + 2 : s + 1);
    consume(a1, b1, s + 1);
  }
#pragma unroll
  for (int I = 0; I < NRT; ++I) {
    double* o = part + ((((long long)blockIdx.x * NRT + I) * n_ct + ct) * 2) * 256;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double s1 = acc[0][I][0][r] + acc[1][I][0][r], s2 = acc[0][I][1][r] + acc[1][I][1][r], s3 = acc[0][I][2][r] + acc[1][I][2][r];
      o[r * 64 + lane] = s1 + s2;
      o[256 + r * 64 + lane] = (s3 - s1) + s2;
    }
  }
  if (is_y) ppow[((long long)blockIdx.x * (n_ct - NRT) + (ct - NRT)) * 64 + lane] = pw;
}

// Fixed-order sum of the chunks' partials: block b < n_rt n_ct -> tile (I, ct) of [G | B] (leading dimension 32; G in columns 0 .. 31, B from column 32 on), the last block
// -> power_in [A].  f64 MFMA C/D layout: row = (lane >> 4) + 4 reg, col = lane & 15.
__global__ __launch_bounds__(256) void ref_reduce_kernel(const double* __restrict__ part, const double* __restrict__ ppow, int n_chunks, int n_rt, int n_ct, int A,
                                                         c64* __restrict__ GB, double* __restrict__ pin) {
  const int b = blockIdx.x, e = threadIdx.x;
  if (b == n_rt * n_ct) {
    const int n_yt = n_ct - n_rt;
    for (int a = e; a < A; a += 256) {
      double s = 0.0;
      for (int c = 0; c < n_chunks; ++c)
#pragma unroll
        for (int kq = 0; kq < 4; ++kq) s += ppow[((long long)c * n_yt + (a >> 4)) * 64 + kq * 16 + (a & 15)];
      pin[a] = s;
    }
    return;
  }
  const int I = b / n_ct, ct = b - I * n_ct;
  double sr = 0.0, si = 0.0;
#pragma unroll 8
  for (int c = 0; c < n_chunks; ++c) {
    const double* o = part + ((((long long)c * n_rt + I) * n_ct + ct) * 2) * 256;
    sr += o[e];
    si += o[256 + e];
  }
  const int r = e >> 6, lane = e & 63;
  const int row = 16 * I + (lane >> 4) + 4 * r, col = lane & 15;
  if (ct < n_rt) GB[row + kRefLd * (16 * ct + col)] = mk(sr, si);
  else if (16 * (ct - n_rt) + col < A) GB[row + kRefLd * (kRefLd + 16 * (ct - n_rt) + col)] = mk(sr, si);
}

// ---------------------------------------------------------------- 2. the solve
// One workgroup.  The lower triangle of G (real diagonal, loaded) -> LDS; right-looking Cholesky G = L L^H in input order with the dependence test on every pivot; then thread a
// solves L y = B[:, a], L^H x = y in place in C[:, a].  rec->dependent: the first dependent reference, or -1.
__global__ __launch_bounds__(256) void ref_solve_kernel(const c64* __restrict__ GB, int M, int A, double loading, c64* __restrict__ C /* [32 x A] */, RefRecord* __restrict__ rec) {
  __shared__ c64 s_l[kRefLd * kRefLd];     // s_l[i + 32 j], i >= j
  __shared__ double s_d0[kRefLd];
  __shared__ int s_dep;
  const int tid = threadIdx.x;
  for (int idx = tid; idx < kRefLd * kRefLd; idx += 256) {
    const int i = idx & (kRefLd - 1), j = idx >> 5;
    c64 v = mk(0.0, 0.0);
    if (i < M && j <= i) {
      v = GB[i + kRefLd * j];
      if (i == j) { v = mk(v.re * (1.0 + loading), 0.0); s_d0[i] = v.re; }
    }
    s_l[idx] = v;
  }
  if (tid == 0) s_dep = -1;
  __syncthreads();
  for (int k = 0; k < M; ++k) {
    const double piv = s_l[k + kRefLd * k].re;
    if (!(piv > kDependentPivot * s_d0[k])) {                              // (uniform: every thread reads the same two values; a NaN is dependent too)
      if (tid == 0) s_dep = k;
      break;
    }
    const double lkk = sqrt(piv);
    __syncthreads();                                                       // every thread has read the pivot
    if (tid == 0) s_l[k + kRefLd * k] = mk(lkk, 0.0);
    if (tid > k && tid < M) s_l[tid + kRefLd * k] = s_l[tid + kRefLd * k] * (1.0 / lkk);
    __syncthreads();
    for (int idx = tid; idx < kRefLd * kRefLd; idx += 256) {
      const int i = idx & (kRefLd - 1), j = idx >> 5;
      if (j > k && j <= i && i < M) s_l[idx] = s_l[idx] - mul_conj(s_l[i + kRefLd * k], s_l[j + kRefLd * k]);
    }
    __syncthreads();
  }
  __syncthreads();
  const int dep = s_dep;
  if (tid == 0) rec->dependent = dep;
  if (dep >= 0) return;
  for (int a = tid; a < A; a += 256) {
    c64* x = C + (long long)kRefLd * a;
    const c64* bcol = GB + (long long)kRefLd * (kRefLd + a);
    for (int i = 0; i < M; ++i) {
      c64 v = bcol[i];
      for (int j = 0; j < i; ++j) v = v - s_l[i + kRefLd * j] * x[j];
      x[i] = v * (1.0 / s_l[i + kRefLd * i].re);
    }
    for (int i = M - 1; i >= 0; --i) {
      c64 v = x[i];
      for (int j = i + 1; j < M; ++j) v = v - conj(s_l[j + kRefLd * i]) * x[j];
      x[i] = v * (1.0 / s_l[i + kRefLd * i].re);
    }
  }
}

// ---------------------------------------------------------------- 3. the subtraction
// Grid (long-lived workgroups over blocks of 256 samples, groups of 16 receive elements).  A thread holds the M reference values of its sample in registers and walks the
// group's elements: Y'[t, a] = Y[t, a] - sum_m R[m, t] C[m, a], references ascending, C in LDS.  The element it reads is the element it writes (in place is safe), and
// |Y'|^2 of the value written goes into the thread's running sum of that element; at the end the workgroup's sums (wave by shuffles, the four waves in order) are one row of
// opart.  A refused solve: nothing is written.
template <int MP>
__global__ __launch_bounds__(256) void ref_subtract_kernel(const c64* __restrict__ R, const c64* Y, c64* out, long long T, int M, int A, const c64* __restrict__ C,
                                                           const RefRecord* __restrict__ rec, double* __restrict__ opart /* [gridDim.x][A] */) {
  __shared__ c64 s_c[kSubCols * MP];
  __shared__ double s_w[4][kSubCols];
  if (rec->dependent >= 0) return;                                         // (uniform, before any barrier)
  const int tid = threadIdx.x;
  const int a0 = blockIdx.y * kSubCols;
  const int na = std::min(kSubCols, A - a0);
  for (int idx = tid; idx < kSubCols * MP; idx += 256) {
    const int j = idx / MP, m = idx - j * MP;
    s_c[idx] = (m < M && j < na) ? C[m + (long long)kRefLd * (a0 + j)] : mk(0.0, 0.0);
  }
  __syncthreads();
  double pw[kSubCols];
#pragma unroll
  for (int j = 0; j < kSubCols; ++j) pw[j] = 0.0;
  for (long long t0 = (long long)blockIdx.x * 256; t0 < T; t0 += (long long)gridDim.x * 256) {
    asm volatile("" ::: "memory");                                         // C is re-read from LDS for every block: hoisted out of this loop it is 32 MP registers and spills
    const long long t = t0 + tid;
    const bool ok = t < T;
    const long long tc = ok ? t : T - 1;
    c64 r[MP];
#pragma unroll
    for (int m = 0; m < MP; ++m) r[m] = m < M ? R[(long long)m * T + tc] : mk(0.0, 0.0);
#pragma unroll
    for (int j = 0; j < kSubCols; ++j) {
      if (j >= na) continue;                                               // (uniform)
      const long long at = (long long)(a0 + j) * T + tc;
      c64 v = Y[at];
#pragma unroll
      for (int m = 0; m < MP; ++m) {
        const c64 cm = s_c[j * MP + m];
        v.re = ::fma(-r[m].re, cm.re, ::fma(r[m].im, cm.im, v.re));
        v.im = ::fma(-r[m].re, cm.im, ::fma(-r[m].im, cm.re, v.im));
      }
      if (ok) {
        out[at] = v;
        pw[j] += v.re * v.re + v.im * v.im;
      }
    }
  }
  const int lane = tid & 63, wid = tid >> 6;
#pragma unroll
  for (int j = 0; j < kSubCols; ++j) {
    double s = pw[j];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64);
    if (lane == 0) s_w[wid][j] = s;
  }
  __syncthreads();
  if (tid < na) opart[(long long)blockIdx.x * A + a0 + tid] = ((s_w[0][tid] + s_w[1][tid]) + s_w[2][tid]) + s_w[3][tid];
}

// power_out by a fixed-order sum over the subtract workgroups; coef and power behind the record's header (success only)
__global__ __launch_bounds__(256) void ref_finish_kernel(RefRecord* __restrict__ rec, const c64* __restrict__ C, const double* __restrict__ pin, const double* __restrict__ opart,
                                                         int n_wg, int M, int A) {
  if (rec->dependent >= 0) return;
  c64* coef = reinterpret_cast<c64*>(rec + 1);
  double* power = reinterpret_cast<double*>(coef + (long long)M * A);
  for (int idx = threadIdx.x; idx < M * A; idx += 256) {
    const int a = idx / M, m = idx - a * M;
    coef[idx] = C[m + (long long)kRefLd * a];
  }
  for (int a = threadIdx.x; a < A; a += 256) {
    double s = 0.0;
    for (int g = 0; g < n_wg; ++g) s += opart[(long long)g * A + a];
    power[a] = pin[a];
    power[A + a] = s;
  }
}

}  // namespace isac

using namespace isac;

extern "C" int isac_cancel_paths_dev(isac_ctx* ctx, const isac_c64* const* d_tx_waves, const int32_t* n_ants_src, int32_t n_sources, int64_t T, double fc, double fs, int32_t n_ants,
                                     int32_t n_refs, const int32_t* ref_source, const int64_t* ref_shift, const double* ref_doppler_hz, const isac_c64* ref_tx_steering,
                                     double loading, const isac_c64* d_rx_wave, isac_c64* d_out, isac_c64* coef, double* power, int32_t* dependent) {
  ISAC_ENTER(ctx);
  const int M = n_refs, A = n_ants;
  if (!d_tx_waves || !n_ants_src || !d_rx_wave || !d_out) return fail(ctx, ISAC_ERR_INVALID_ARG, "NULL argument");
  if (T <= 0 || A <= 0 || n_sources <= 0 || M <= 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "bad T / n_ants / n_sources / n_refs");
  if (!(fs > 0)) return fail(ctx, ISAC_ERR_INVALID_ARG, "fs must be positive");
  if (!(loading >= 0) || !std::isfinite(loading)) return fail(ctx, ISAC_ERR_INVALID_ARG, "loading must be finite and >= 0");
  if (M > ISAC_CANCEL_PATHS_MAX_REFS) return fail(ctx, ISAC_ERR_CAPACITY, "more than 32 references");
  if (n_sources > ISAC_MULTISTATIC_MAX_SOURCES) return fail(ctx, ISAC_ERR_CAPACITY, "more than 32 sources");
  if (A > ISAC_MULTISTATIC_MAX_ANTS) return fail(ctx, ISAC_ERR_CAPACITY, "more than 256 receive elements");
  if (!ref_source || !ref_shift || !ref_doppler_hz || !ref_tx_steering) return fail(ctx, ISAC_ERR_INVALID_ARG, "NULL argument");
  for (int m = 0; m < M; ++m) {
    const int s = ref_source[m];
    if (s < 0 || s >= n_sources) return fail(ctx, ISAC_ERR_INVALID_ARG, "ref_source outside 0 .. n_sources - 1");
    if (ref_shift[m] < 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "negative ref_shift");
    if (!d_tx_waves[s] || n_ants_src[s] <= 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "a reference names a source without a waveform");
    if (n_ants_src[s] > ISAC_MULTISTATIC_MAX_ANTS) return fail(ctx, ISAC_ERR_CAPACITY, "more than 256 elements on a source array");
  }
  const size_t wave_bytes = sizeof(c64) * (size_t)T * A;
  if ((const void*)d_out != (const void*)d_rx_wave) {
    const char *x = (const char*)d_rx_wave, *o = (const char*)d_out;
    if (o < x + wave_bytes && x < o + wave_bytes) return fail(ctx, ISAC_ERR_INVALID_ARG, "d_out partially overlaps d_rx_wave");
  }
  // an echo call: the reference columns are formed in the echo calls' scratch
  ctx->range_cache.valid = false;
  ctx->lazy.valid = false;
  const std::vector<double> unit_gain(M, 1.0);
  const std::vector<isac_c64> unit_rx(M, isac_c64{1.0, 0.0});               // one receive element: [1 x M]
  const PathCoefJob job{(const c64* const*)d_tx_waves, n_ants_src, T, fc, fs, 1, M, ref_source, ref_shift, ref_doppler_hz, unit_gain.data(), ref_tx_steering, unit_rx.data()};
  ISAC_TRY(isac_path_coefs_on(ctx, ctx->stream, job));
  const c64* R = (const c64*)ctx->coef.p;

  const int n_rt = (M + 15) / 16, n_yt = (A + 15) / 16, n_ct = n_rt + n_yt, n_cg = (n_ct + 3) / 4;
  const long long slabs = (T + 15) / 16;
  long long n_chunks = std::min<long long>(slabs, std::max(1, 1024 / n_cg));
  const long long per = (slabs + n_chunks - 1) / n_chunks;
  n_chunks = (slabs + per - 1) / per;
  int n_cus = 0;
  ISAC_TRY(ctx_n_cus(ctx, &n_cus));
  const int n_ag = (A + kSubCols - 1) / kSubCols;
  const long long n_sub = std::min<long long>(cdiv(T, 256), std::max(1, 8 * n_cus / n_ag));
  // scratch: [partial tiles | power partials | G | B | power_in | C | subtract partials | record]
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t off_part = 0;
  const size_t off_ppow = off_part + up(sizeof(double) * (size_t)n_chunks * n_rt * n_ct * 2 * 256);
  const size_t off_gb = off_ppow + up(sizeof(double) * (size_t)n_chunks * n_yt * 64);
  const size_t off_pin = off_gb + up(sizeof(c64) * (size_t)kRefLd * (kRefLd + A));
  const size_t off_c = off_pin + up(sizeof(double) * (size_t)A);
  const size_t off_opart = off_c + up(sizeof(c64) * (size_t)kRefLd * A);
  const size_t off_rec = off_opart + up(sizeof(double) * (size_t)n_sub * A);
  const size_t rec_bytes = sizeof(RefRecord) + sizeof(c64) * (size_t)M * A + sizeof(double) * 2 * (size_t)A;
  ISAC_TRY(ensure(ctx, ctx->cancel_paths, off_rec + up(rec_bytes)));
  char* base = (char*)ctx->cancel_paths.p;
  double* part = (double*)(base + off_part);
  double* ppow = (double*)(base + off_ppow);
  c64* GB = (c64*)(base + off_gb);
  double* pin = (double*)(base + off_pin);
  c64* Cd = (c64*)(base + off_c);
  double* opart = (double*)(base + off_opart);
  RefRecord* rec = (RefRecord*)(base + off_rec);

  const dim3 gg((unsigned)n_chunks, (unsigned)n_cg);
  if (n_rt == 1) hipLaunchKernelGGL(ref_gram_kernel<1>, gg, dim3(256), 0, ctx->stream, R, (const c64*)d_rx_wave, (long long)T, M, A, per, n_ct, part, ppow);
  else           hipLaunchKernelGGL(ref_gram_kernel<2>, gg, dim3(256), 0, ctx->stream, R, (const c64*)d_rx_wave, (long long)T, M, A, per, n_ct, part, ppow);
  ISAC_HIP(hipGetLastError());
  hipLaunchKernelGGL(ref_reduce_kernel, dim3(n_rt * n_ct + 1), dim3(256), 0, ctx->stream, (const double*)part, (const double*)ppow, (int)n_chunks, n_rt, n_ct, A, GB, pin);
  ISAC_HIP(hipGetLastError());
  hipLaunchKernelGGL(ref_solve_kernel, dim3(1), dim3(256), 0, ctx->stream, (const c64*)GB, M, A, loading, Cd, rec);
  ISAC_HIP(hipGetLastError());
  const dim3 gs((unsigned)n_sub, (unsigned)n_ag);
  auto sub = [&](auto mp) {
    hipLaunchKernelGGL(ref_subtract_kernel<decltype(mp)::value>, gs, dim3(256), 0, ctx->stream, R, (const c64*)d_rx_wave, (c64*)d_out, (long long)T, M, A, (const c64*)Cd,
                       (const RefRecord*)rec, opart);
  };
  if (M <= 8) sub(std::integral_constant<int, 8>{});
  else if (M <= 16) sub(std::integral_constant<int, 16>{});
  else sub(std::integral_constant<int, 32>{});
  ISAC_HIP(hipGetLastError());
  hipLaunchKernelGGL(ref_finish_kernel, dim3(1), dim3(256), 0, ctx->stream, rec, (const c64*)Cd, (const double*)pin, (const double*)opart, (int)n_sub, M, A);
  ISAC_HIP(hipGetLastError());

  std::vector<char> host(rec_bytes);
  ISAC_TRY(copy_d2h(ctx, host.data(), rec, rec_bytes));                    // the one read-back: waits for the stream
  RefRecord hdr;
  std::memcpy(&hdr, host.data(), sizeof(hdr));
  if (dependent) *dependent = hdr.dependent;
  if (hdr.dependent >= 0)
    return fail(ctx, ISAC_ERR_INVALID_ARG, "reference " + std::to_string(hdr.dependent) + " is dependent on the references before it (or all zero): nothing was subtracted");
  if (coef) std::memcpy(coef, host.data() + sizeof(hdr), sizeof(c64) * (size_t)M * A);
  if (power) std::memcpy(power, host.data() + sizeof(hdr) + sizeof(c64) * (size_t)M * A, sizeof(double) * 2 * (size_t)A);
  return ISAC_OK;
}
