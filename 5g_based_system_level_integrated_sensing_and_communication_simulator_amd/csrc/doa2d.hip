// 2-D (elevation x azimuth) DoA scan of a uniform planar array and the project's find2DPeaks (gfx950 only).
// music.m:31-71, digitalBF.m:13-53, mvdrBF.m:13-53: every point of the [eSteps x aSteps] grid is
//   P_j = sum_i w_i |v_i' a_j|^2          (eigenpairs (lambda_i, v_i) of Ra; DBF w = lambda, MVDR w = 1/lambda, MUSIC w = [rank >= L])
// or, on MUSIC's signal-subspace route, || a_j - Us Us' a_j ||^2; then the column normalisation of music.m:61-63 and the strict
// 8-neighbour maxima (include/isac.h, isac_find2d_peaks).  Own translation unit: the echo / eigh / music / cdl code objects stay as they are.
#include <algorithm>
#include <vector>

#include "isac_internal.hpp"
#include "upa_steer.hpp"

using namespace isac;

namespace {

constexpr int kThreads = 256;
constexpr int kCandHdr = 2;          // doubles in front of the candidate pairs: [0] holds the 32-bit candidate counter

// the L signal vectors of music_subspace_kernel are delivered when ctl[kRoute] == 1 (ctl[kLsub] of them)
__device__ __forceinline__ bool subspace_delivered(const int* ctl) { return ctl && ctl[MusicCtl::kRoute] == 1; }

// per-eigenpair weight: MUSIC (mode 0) 1 for the noise subspace (descending rank >= L, ties in index order, as music_scan_kernel),
// 0 for the signal subspace; DBF (mode 1) lambda; MVDR (mode 2) 1 / lambda
__global__ __launch_bounds__(kThreads) void doa2d_weights_kernel(const double* __restrict__ w, int A, int mode, const int* __restrict__ num_dets_dev,
                                                                 int num_dets_host, double* __restrict__ wgt) {
  const int Lsig = num_dets_dev ? *num_dets_dev : num_dets_host;
  for (int v = threadIdx.x; v < A; v += blockDim.x) {
    const double wv = w[v];
    double weight;
    if (mode == 0) {
      int rank = 0;
      for (int j = 0; j < A; ++j) rank += (w[j] > wv || (w[j] == wv && j < v)) ? 1 : 0;
      weight = rank < Lsig ? 0.0 : 1.0;
    } else {
      weight = mode == 1 ? wv : 1.0 / wv;
    }
    wgt[v] = weight;
  }
}

// One workgroup per tile of PT scan points (j = e + eSteps a, column-major like the reference's P(e, a)).  The steering tile [A x PT]
// is formed in LDS from the three host tables (upa_steer, upa_steer.hpp), the phase in ONE association for every point:
//     arg = ((-2 pi) sind(th)) * fma(m d, cosd(ph), (n d) sind(ph)),    element r = n + nH m   (music.m:44-55)
// so that mirror twins (ph -+ 180, -th) -- whose table entries are exact negatives -- get bitwise equal vectors.  Every point then takes
// the same reduction order (sum over m ascending, over the thread's four vectors in order, over the vector groups in order), wherever it
// sits in its tile: equal vectors give equal values.
// Weighted modes: thread (pg, vg) owns points 4 pg .. 4 pg + 3 and eigenvectors 4 vg .. 4 vg + 3 (4 VG = 4096 / PT >= A: one pass).
// Subspace route: y = Us' a into LDS (the Ls <= 32 signal vectors), then r = a - Us y per element and the sum of |r|^2 over
// (256 / PT) element groups -- a sum of squares, no cancellation at the peaks (music.hip: music_scan_kernel).
template <int PT>
__global__ __launch_bounds__(kThreads) void doa2d_scan_kernel(const double* __restrict__ tab, int eS, int aS, int nV, int nH,
                                                              const c64* __restrict__ V, const double* __restrict__ wgt, int mode,
                                                              const int* __restrict__ ctl, double eps1, double* __restrict__ p_out) {
  constexpr int PG = PT / 4, VG = kThreads / PG, G2 = kThreads / PT;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int A = nV * nH;
  const int n_pts = eS * aS;
  c64* s_a = reinterpret_cast<c64*>(smem_raw);                       // [A][PT]
  double* s_part = reinterpret_cast<double*>(s_a + (size_t)A * PT);  // [VG][PT]
  c64* s_y = reinterpret_cast<c64*>(s_part + VG * PT);               // [Ls][PT] (subspace route only)
  const int tid = threadIdx.x;
  const int j0 = blockIdx.x * PT;
  for (int t = tid; t < A * PT; t += kThreads) {
    const int p = t % PT, r = t / PT;
    s_a[t] = upa_steer(tab, eS, aS, nH, min(j0 + p, n_pts - 1), r);   // (tail points repeat the last one; not stored)
  }
  __syncthreads();
  double t_out = 0.0;
  if (mode == 0 && subspace_delivered(ctl)) {
    const int Ls = ctl[MusicCtl::kLsub];
    if (Ls < A) {                                                    // (Ls >= A: empty noise space, the quadratic form is 0)
      const int pg = tid % PG, vg = tid / PG, i0 = 4 * vg;
      if (i0 < Ls) {
        c64 y[4][4];
        for (int k = 0; k < 4; ++k)
          for (int q = 0; q < 4; ++q) y[k][q] = mk(0.0, 0.0);
        for (int m = 0; m < A; ++m) {
          c64 av[4], vv[4];
          for (int q = 0; q < 4; ++q) av[q] = s_a[m * PT + 4 * pg + q];
          for (int k = 0; k < 4; ++k) vv[k] = V[m + (long long)A * min(i0 + k, Ls - 1)];
          for (int k = 0; k < 4; ++k)
            for (int q = 0; q < 4; ++q) y[k][q] = fma(conj(vv[k]), av[q], y[k][q]);
        }
        for (int k = 0; k < 4; ++k)
          if (i0 + k < Ls)
            for (int q = 0; q < 4; ++q) s_y[(i0 + k) * PT + 4 * pg + q] = y[k][q];
      }
      __syncthreads();
      const int p = tid % PT, g = tid / PT;
      double acc = 0.0;
      for (int m = g; m < A; m += G2) {
        c64 r = s_a[m * PT + p];
        for (int sv = 0; sv < Ls; ++sv) r = r - V[m + (long long)A * sv] * s_y[sv * PT + p];
        acc = ::fma(r.re, r.re, ::fma(r.im, r.im, acc));
      }
      s_part[g * PT + p] = acc;
      __syncthreads();
      if (tid < PT)
        for (int gg = 0; gg < G2; ++gg) t_out += s_part[gg * PT + tid];
    }
  } else {
    const int pg = tid % PG, vg = tid / PG, i0 = 4 * vg;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (i0 < A) {
      c64 y[4][4];
      for (int k = 0; k < 4; ++k)
        for (int q = 0; q < 4; ++q) y[k][q] = mk(0.0, 0.0);
      for (int m = 0; m < A; ++m) {
        c64 av[4], vv[4];
        for (int q = 0; q < 4; ++q) av[q] = s_a[m * PT + 4 * pg + q];
        for (int k = 0; k < 4; ++k) vv[k] = V[m + (long long)A * min(i0 + k, A - 1)];
        for (int k = 0; k < 4; ++k)
          for (int q = 0; q < 4; ++q) y[k][q] = fma(conj(vv[k]), av[q], y[k][q]);
      }
      for (int k = 0; k < 4; ++k) {
        if (i0 + k >= A) break;
        const double wk = wgt[i0 + k];
        for (int q = 0; q < 4; ++q) acc[q] += wk * (y[k][q].re * y[k][q].re + y[k][q].im * y[k][q].im);
      }
    }
    for (int q = 0; q < 4; ++q) s_part[vg * PT + 4 * pg + q] = acc[q];
    __syncthreads();
    if (tid < PT)
      for (int g = 0; g < VG; ++g) t_out += s_part[g * PT + tid];
  }
  if (tid < PT && j0 + tid < n_pts)
    p_out[j0 + tid] = mode == 1 ? t_out : 1.0 / (t_out + eps1);    // digitalBF.m:38 / music.m:56, mvdrBF.m:38
}

// music.m:61-63 on a matrix: P = -abs(P); PNorm = P ./ max(P) (COLUMN maxima, i.e. each column over its least magnitude); mag2db.
// One workgroup per azimuth column.
__global__ __launch_bounds__(kThreads) void doa2d_norm_kernel(const double* __restrict__ P, int eS, double* __restrict__ db) {
  __shared__ double s_min[kThreads / 64];
  const int a = blockIdx.x, tid = threadIdx.x;
  const double* col = P + (long long)eS * a;
  double mn = INFINITY;
  for (int e = tid; e < eS; e += kThreads) mn = fmin(mn, fabs(col[e]));
  for (int o = 32; o > 0; o >>= 1) mn = fmin(mn, __shfl_down(mn, o));
  if ((tid & 63) == 0) s_min[tid >> 6] = mn;
  __syncthreads();
  mn = s_min[0];
  for (int i = 1; i < kThreads / 64; ++i) mn = fmin(mn, s_min[i]);
  for (int e = tid; e < eS; e += kThreads) db[(long long)eS * a + e] = 20.0 * log10((-fabs(col[e])) / (-mn));
}

// find2DPeaks, device half: interior cells strictly above all 8 neighbours (a NaN is never a peak) -> (value, linear index) pairs,
// compacted through a vector atomic counter.  cap bounds the stores; the host reports a count above cap.
__global__ __launch_bounds__(kThreads) void doa2d_peaks_kernel(const double* __restrict__ db, int rows, int cols, double* __restrict__ cand, int cap) {
  const long long n_in = (long long)(rows - 2) * (cols - 2);
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_in) return;
  const int e = 1 + (int)(t % (rows - 2)), a = 1 + (int)(t / (rows - 2));
  const long long j = e + (long long)rows * a;
  const double v = db[j];
  bool peak = true;
  for (int da = -1; da <= 1; ++da)
    for (int de = -1; de <= 1; ++de)
      if (da != 0 || de != 0) peak = peak && v > db[j + de + (long long)rows * da];
  if (!peak) return;
  const unsigned slot = atomicAdd(reinterpret_cast<unsigned*>(cand), 1u);
  if ((int)slot < cap) {
    cand[kCandHdr + 2 * (long long)slot] = v;
    cand[kCandHdr + 2 * (long long)slot + 1] = (double)j;
  }
}

}  // namespace

// ------------------------------------------------------------------ host side (called from doa.hip)
// at most one strict maximum in every 2 x 2 block of the interior
int isac_doa2d_peak_cap(int rows, int cols) {
  if (rows < 3 || cols < 3) return 0;
  return ((rows - 2 + 1) / 2) * ((cols - 2 + 1) / 2);
}
int isac_doa2d_cand_doubles(int cap) { return kCandHdr + 2 * (cap > 0 ? cap : 1); }

// P [eS x aS] into ctx->doa2d_p from the eigenpairs in ctx->eig_w / eig_v (or the signal vectors, when ctl says they were delivered).
// d_tab: [sind(ele) eS | cosd(azi) aS | sind(azi) aS].  L from d_num_dets (device) or num_dets_host.
int isac_doa2d_scan_dev(isac_ctx* ctx, int mode, int nV, int nH, int eS, int aS, const double* d_tab, const int* d_num_dets, int num_dets_host,
                        const int* ctl, hipStream_t st) {
  if (!st) st = ctx->stream;
  const int A = nV * nH;
  if (A < 1 || A > 256) return fail(ctx, ISAC_ERR_UNSUPPORTED, "UPA DoA: the 2-D scan supports 1..256 elements");
  const long long n_pts = (long long)eS * aS;
  if (eS <= 0 || aS <= 0 || n_pts > (1ll << 30)) return fail(ctx, ISAC_ERR_INVALID_ARG, "UPA DoA: empty or oversized scan grid");
  ISAC_TRY(ensure(ctx, ctx->doa2d_p, sizeof(double) * (size_t)n_pts));
  ISAC_TRY(ensure(ctx, ctx->doa2d_w, sizeof(double) * (size_t)A));
  // (also on the subspace route: when L exceeds what the subspace kernel holds, its QL fallback delivers the full basis and the scan weighs it)
  hipLaunchKernelGGL(doa2d_weights_kernel, dim3(1), dim3(kThreads), 0, st, (const double*)ctx->eig_w.p, A, mode, d_num_dets, num_dets_host,
                     (double*)ctx->doa2d_w.p);
  ISAC_HIP(hipGetLastError());
  if (mode != 0) ctl = nullptr;
  const double eps1 = 2.220446049250313e-16;                        // eps(1)
#define ISAC_SCAN2D(PT_)                                                                                                        \
  do {                                                                                                                          \
    const size_t lds = sizeof(c64) * (size_t)A * PT_ + sizeof(double) * (size_t)(kThreads / (PT_ / 4)) * PT_ +                  \
                       (ctl ? sizeof(c64) * 32 * PT_ : 0);                                                                      \
    ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(doa2d_scan_kernel<PT_>), lds));                                      \
    hipLaunchKernelGGL(doa2d_scan_kernel<PT_>, dim3((unsigned)((n_pts + PT_ - 1) / PT_)), dim3(kThreads), lds, st, d_tab, eS, aS, \
                       nV, nH, (const c64*)ctx->eig_v.p, (const double*)ctx->doa2d_w.p, mode, ctl, eps1, (double*)ctx->doa2d_p.p); \
  } while (0)
  if (A <= 64) ISAC_SCAN2D(64); else if (A <= 128) ISAC_SCAN2D(32); else ISAC_SCAN2D(16);
#undef ISAC_SCAN2D
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}

// music.m:61-63 + the device half of find2DPeaks: ctx->doa2d_p -> ctx->doa2d_db (normalise == true), then the candidates of d_db
// into d_cand ([counter | pairs], cap pairs).
int isac_doa2d_norm_peaks_dev(isac_ctx* ctx, bool normalise, const double* d_db, int rows, int cols, double* d_cand, int cap, hipStream_t st) {
  if (!st) st = ctx->stream;
  if (normalise) {
    hipLaunchKernelGGL(doa2d_norm_kernel, dim3((unsigned)cols), dim3(kThreads), 0, st, (const double*)ctx->doa2d_p.p, rows, (double*)d_db);
    ISAC_HIP(hipGetLastError());
  }
  ISAC_HIP(hipMemsetAsync(d_cand, 0, sizeof(double) * kCandHdr, st));
  const long long n_in = rows >= 3 && cols >= 3 ? (long long)(rows - 2) * (cols - 2) : 0;
  if (n_in > 0) {
    hipLaunchKernelGGL(doa2d_peaks_kernel, dim3((unsigned)((n_in + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, d_db, rows, cols, d_cand, cap);
    ISAC_HIP(hipGetLastError());
  }
  return ISAC_OK;
}

// find2DPeaks, host half: stable descending sort of the candidates in column-major index order (include/isac.h), the first min(L, #) as
// 1-based (ele, azi).  cand: [counter | pairs] as the device left it; returns ISAC_ERR_HIP when the counter exceeds cap.
int isac_doa2d_select(isac_ctx* ctx, const double* cand, int count, int cap, int rows, int L, std::vector<int>& ele, std::vector<int>& azi) {
  ele.clear();
  azi.clear();
  if (count < 0 || count > cap) return fail(ctx, ISAC_ERR_HIP, "find2DPeaks: candidate count beyond the 2 x 2 bound (internal error)");
  std::vector<std::pair<double, long long>> c((size_t)count);
  for (int i = 0; i < count; ++i) c[(size_t)i] = {cand[kCandHdr + 2 * i], (long long)cand[kCandHdr + 2 * i + 1]};
  std::sort(c.begin(), c.end(), [](const std::pair<double, long long>& x, const std::pair<double, long long>& y) {
    return x.first > y.first || (x.first == y.first && x.second < y.second);
  });
  const int n = std::min(L, count);
  for (int i = 0; i < n; ++i) {
    ele.push_back((int)(c[(size_t)i].second % rows) + 1);
    azi.push_back((int)(c[(size_t)i].second / rows) + 1);
  }
  return ISAC_OK;
}
