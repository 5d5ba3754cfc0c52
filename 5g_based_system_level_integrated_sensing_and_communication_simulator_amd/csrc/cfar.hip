// The other detectors of phased.CFARDetector2D (gfx950 only): cell averaging, greatest-of / smallest-of cell averaging and ordered statistics, with the automatic or a
// custom threshold factor (cfar2D.m:28-29 names them; include/isac_cfar.h and DESIGN.md section 5 define what the toolbox leaves open).  Entry points:
//   isac_cfar_threshold_factor   host only: the 'Auto' factor of a method
//   isac_cfar2d                  an arbitrary map and CUT list (isac_cfar2d_ca with the method block)
//   isac_fft2d_redetect          the power window of the last completed fft2D, detected again; then the host half of fft2D.m:63-99 on the new lists
//   cfar_detect_planes           (internal) the device half of isac_fft2d_redetect on any planes with the window's geometry: also the detector of isac_fft2d_beam_detect (beams.hip)
//   isac_cfar_monte_carlo        (include/isac_cfar_mc.h) drawn noise and a target through the same per-CUT function, counted: the detectors' Pfa / Pd as built
// One per-CUT device function, cfar_cut<M>, serves both: K1 cfar_method_window_kernel stages a kPanelRows x pc tile of CUTs plus its halo of guard + training cells in LDS
// and evaluates one CUT per lane into a flag per (CUT, antenna); K2 cfar_compact_kernel, one workgroup per antenna, turns the flags into the CUT-order list (rows
// fastest, cfar2D.m:23-24) with ballots and a running base; cfar_method_list_kernel evaluates one listed CUT per lane on a map in global memory.  The CA detector of the
// timed fft2D path (rdm.hip) is not touched; cfar_cut<CA> restates its arithmetic operation for operation.  Everything here is off the timed path.
#include <algorithm>
#include <cmath>

#include "isac_internal.hpp"
#include "echo_dev.hpp"

namespace isac {

struct CutGeom {
  int hr, hc;          // guard + training half sizes
  int gr, gc;          // guard half sizes
  int n_train;         // N
  int rank;            // OS: 1..N
  double alpha;
};

// ---------------------------------------------------------------- one CUT: cutp points at the CUT, the cell (dr, dc) away is cutp[dr + dc * ld].  LDS or global memory.
// Training cells in the ORACLE-DEFINED order of the CA kernels (column offset slowest, row offset fastest, guard block skipped; oracle/cfar.py); correctly rounded
// operations only, so the flag is a function of the map's bits.
template <int M>
__device__ __forceinline__ bool cfar_cut(const double* __restrict__ cutp, int ld, const CutGeom& g) {
  double est;
  if constexpr (M == ISAC_CFAR_CA) {
    double acc = 0.0;
    for (int dc = -g.hc; dc <= g.hc; ++dc) {
      const bool guard_col = (dc >= -g.gc && dc <= g.gc);
      const double* colp = cutp + (long long)dc * ld;
      for (int dr = -g.hr; dr <= g.hr; ++dr) {
        if (guard_col && dr >= -g.gr && dr <= g.gr) continue;
        acc = __dadd_rn(acc, colp[dr]);
      }
    }
    est = __ddiv_rn(acc, (double)g.n_train);
  } else if constexpr (M == ISAC_CFAR_GOCA || M == ISAC_CFAR_SOCA) {
    const int half = g.n_train / 2;                             // front half: the cells before the CUT in this order
    double front = 0.0, rear = 0.0;
    int k = 0;                                                  // (uniform over the lanes: no divergence)
    for (int dc = -g.hc; dc <= g.hc; ++dc) {
      const bool guard_col = (dc >= -g.gc && dc <= g.gc);
      const double* colp = cutp + (long long)dc * ld;
      for (int dr = -g.hr; dr <= g.hr; ++dr) {
        if (guard_col && dr >= -g.gr && dr <= g.gr) continue;
        if (k < half) front = __dadd_rn(front, colp[dr]);
        else rear = __dadd_rn(rear, colp[dr]);
        ++k;
      }
    }
    front = __ddiv_rn(front, (double)half);
    rear = __ddiv_rn(rear, (double)half);
    est = M == ISAC_CFAR_GOCA ? (front > rear ? front : rear) : (front < rear ? front : rear);
    if (front != front) est = front;                            // a NaN mean is the estimate (the comparisons above drop it): no detection
    if (rear != rear) est = rear;
  } else {
    // the rank-th smallest: the candidate with exactly rank - 1 cells below it, ties broken by index -- a strict total order, so exactly one candidate qualifies.
    // Both loops read the map (LDS in the window kernel); nothing is kept in a per-lane array.
    bool has_nan = false;
    est = 0.0;
    int i = 0;
    for (int dc = -g.hc; dc <= g.hc; ++dc) {
      const bool guard_col = (dc >= -g.gc && dc <= g.gc);
      const double* colp = cutp + (long long)dc * ld;
      for (int dr = -g.hr; dr <= g.hr; ++dr) {
        if (guard_col && dr >= -g.gr && dr <= g.gr) continue;
        const double ti = colp[dr];
        has_nan |= ti != ti;
        int below = 0, j = 0;
        for (int dc2 = -g.hc; dc2 <= g.hc; ++dc2) {
          const bool guard_col2 = (dc2 >= -g.gc && dc2 <= g.gc);
          const double* colp2 = cutp + (long long)dc2 * ld;
          for (int dr2 = -g.hr; dr2 <= g.hr; ++dr2) {
            if (guard_col2 && dr2 >= -g.gr && dr2 <= g.gr) continue;
            const double tj = colp2[dr2];
            below += ((tj < ti) | ((tj == ti) & (j < i))) ? 1 : 0;
            ++j;
          }
        }
        if (below == g.rank - 1) est = ti;
        ++i;
      }
    }
    if (has_nan) est = __builtin_nan("");                       // a rank count skips NaNs: make the rule hold
  }
  const double thr = __dmul_rn(g.alpha, est);
  return *cutp > thr;                                           // strict; a NaN CUT or threshold compares false
}

// ---------------------------------------------------------------- K1: a tile of the CUT rectangle of one antenna, one lane per CUT
constexpr int kPanelRows = 32;                                  // CUT rows per workgroup (the panel height)
constexpr int kPanelColsMax = 8;                                // CUT columns per workgroup: 256 lanes

struct WinGeom {
  int nr, nc;                    // power window dims
  int n_cut_rows, n_cut_cols;
  int cut_row_lo, cut_row_hi;    // the CUT rows this launch evaluates: [cut_row_lo, cut_row_hi) of 0 .. n_cut_rows (all of them, or the band of isac_fft2d_beam_clean_targets)
  int pc;                        // CUT columns per workgroup, 1..kPanelColsMax (from the LDS budget)
  CutGeom c;
};

template <int M>
__global__ __launch_bounds__(kPanelRows * kPanelColsMax) void cfar_method_window_kernel(const double* __restrict__ pwin /* [nr x nc x A] */, WinGeom g,
                                                                                         unsigned char* __restrict__ flags /* [A][n_cut], CUT order */) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* s_p = reinterpret_cast<double*>(smem_raw);            // [pc + 2 hc][kPanelRows + 2 hr], rows fastest
  constexpr int NT = kPanelRows * kPanelColsMax;
  const int tid = threadIdx.x;
  const int r0 = g.cut_row_lo + blockIdx.x * kPanelRows, c0 = blockIdx.y * g.pc, a = blockIdx.z;   // first CUT row / column of the tile = first window row / column staged
  const int wr = kPanelRows + 2 * g.c.hr, wc = g.pc + 2 * g.c.hc;
  {   // 8 independent loads in flight per thread (cells past the window, where the tile overhangs the zone: clamped, never used by a CUT)
    const double* src = pwin + (long long)g.nr * g.nc * a;
    const int n_el = wr * wc;
    for (int i0 = tid; i0 < n_el; i0 += 8 * NT) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = min(i0 + u * NT, n_el - 1);
        const int pcol = i / wr, prow = i - pcol * wr;
        v[u] = src[(long long)min(r0 + prow, g.nr - 1) + (long long)g.nr * min(c0 + pcol, g.nc - 1)];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) { const int i = i0 + u * NT; if (i < n_el) s_p[i] = v[u]; }
    }
  }
  __syncthreads();
  const int crl = tid % kPanelRows, ccl = tid / kPanelRows;     // lanes along a column read consecutive doubles: no bank conflict
  const int cr = r0 + crl, cc = c0 + ccl;
  if (ccl < g.pc && cr < g.cut_row_hi && cc < g.n_cut_cols) {
    const bool det = cfar_cut<M>(s_p + (ccl + g.c.hc) * wr + crl + g.c.hr, wr, g.c);
    flags[(long long)a * g.n_cut_rows * g.n_cut_cols + cr + (long long)g.n_cut_rows * cc] = det ? 1 : 0;
  }
}

// ---------------------------------------------------------------- K2: flags of one antenna -> its list in CUT order, the CUTs' powers, the detected rows
__global__ __launch_bounds__(256) void cfar_compact_kernel(const unsigned char* __restrict__ flags /* [A][n_cut] */, const double* __restrict__ pwin, int nr, int nc,
                                                           int hr, int hc, int n_cut_rows, int n_cut, int* __restrict__ det_cut /* [A][n_cut] CUT ordinal */,
                                                           double* __restrict__ det_pow /* [A][n_cut] */, int* __restrict__ det_cnt /* [A] */,
                                                           unsigned* __restrict__ row_seen /* [n_cut_rows], zeroed */) {
  __shared__ int s_w[4];                                        // detections of each wave in this round
  const int a = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const unsigned char* f = flags + (long long)a * n_cut;
  const double* p = pwin + (long long)nr * nc * a;
  int base = 0;                                                 // detections before this round (every thread keeps the same count)
  for (int i0 = 0; i0 < n_cut; i0 += 256) {
    const int i = i0 + tid;
    const bool det = i < n_cut && f[i] != 0;
    const unsigned long long mask = __ballot(det);
    if (lane == 0) s_w[wid] = __popcll(mask);
    __syncthreads();
    int off = base;
    for (int q = 0; q < wid; ++q) off += s_w[q];
    base += s_w[0] + s_w[1] + s_w[2] + s_w[3];
    if (det) {
      const int pos = off + __popcll(mask & ((1ull << lane) - 1ull));   // < n_cut: at most one entry per CUT
      const int cr = i % n_cut_rows, cc = i / n_cut_rows;
      det_cut[(long long)a * n_cut + pos] = i;
      det_pow[(long long)a * n_cut + pos] = p[(long long)(cr + hr) + (long long)nr * (cc + hc)];
      row_seen[cr] = 1u;                                        // (every writer stores the same value)
    }
    __syncthreads();                                            // s_w is rewritten in the next round
  }
  if (tid == 0) det_cnt[a] = base;
}

// ---------------------------------------------------------------- arbitrary CUT list on an arbitrary map: one lane per listed CUT, the map in global memory
template <int M>
__global__ __launch_bounds__(256) void cfar_method_list_kernel(const double* __restrict__ P, int n_rows, const int* __restrict__ cut /* [2 x n_cut] 1-based */,
                                                               int n_cut, CutGeom g, unsigned char* __restrict__ flags) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_cut) return;
  const int r = cut[2 * i] - 1, c = cut[2 * i + 1] - 1;         // (the host has checked that the training window stays inside the map)
  flags[i] = cfar_cut<M>(P + (long long)r + (long long)n_rows * c, n_rows, g) ? 1 : 0;
}

// ---------------------------------------------------------------- Monte Carlo (include/isac_cfar_mc.h): one lane per trial, the lane's 1 x (N + 1) window in LDS
constexpr int kMcMaxSnr = 64;                                   // SNR points per call = lanes of a wave: lane i of every wave keeps the count of point i
constexpr unsigned long long kMcLaunchTrials = 1ull << 28;      // trials per launch: the host loops, so that no kernel holds the device for long

struct McGeom {
  CutGeom c;                     // hr = 0, hc = N/2, no guard: the CUT in the middle column
  int n_snr, model;
  unsigned long long t0, n;      // this launch: trials t0 .. t0 + n - 1
  unsigned long long n_trials;   // leading dimension of flags
  unsigned long long seed;
};
struct McSnr { double s[kMcMaxSnr], root[kMcMaxSnr]; };         // S_i and sqrt(S_i)

__device__ __forceinline__ double neg_ln_u53(uint64_t w) { return -ln_unit(((double)(w >> 11) + 1.0) * 0x1.0p-53); }   // -ln u(w), u in (0, 1]: a unit-mean exponential

// Cell c of lane l at s_c[c * NT + l]: the lanes of a wave read consecutive doubles in every step of cfar_cut (ld = NT), so no bank conflict.  A lane touches its own column
// only, so no barrier inside the trial loop; the loop bounds are uniform over the workgroup and a lane past the end repeats the launch's last trial without counting it.
template <int M, int NT>
__global__ __launch_bounds__(NT) void cfar_mc_kernel(McGeom g, McSnr snr, unsigned long long* __restrict__ n_det /* [n_snr], zeroed before the first launch */,
                                                     unsigned char* __restrict__ flags /* [n_trials x n_snr] or nullptr */) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  __shared__ unsigned long long s_tot[kMcMaxSnr];
  double* s_c = reinterpret_cast<double*>(smem_raw);            // [N + 1][NT]
  const int tid = threadIdx.x, lane = tid & 63;
  const int half = g.c.n_train / 2;
  if (tid < kMcMaxSnr) s_tot[tid] = 0ull;
  __syncthreads();
  double* cutp = s_c + half * NT + tid;
  const uint32_t k0 = (uint32_t)g.seed, k1 = (uint32_t)(g.seed >> 32);
  unsigned long long cnt = 0ull;                                // detections of SNR point `lane` seen by this wave
  for (unsigned long long base = (unsigned long long)blockIdx.x * NT; base < g.n; base += (unsigned long long)gridDim.x * NT) {
    const bool active = base + tid < g.n;
    const unsigned long long t = g.t0 + (active ? base + tid : g.n - 1);
    uint32_t o[4];
    for (int j = 0; j < half; ++j) {                            // T_{2j+1}, T_{2j+2}: columns 0 .. half - 1 before the CUT, half + 1 .. N after it
      philox4x32_10((uint32_t)t, (uint32_t)(t >> 32), kCfarMcStream, (uint32_t)j, k0, k1, o);
      const int c0 = 2 * j, c1 = 2 * j + 1;
      s_c[(c0 + (c0 >= half ? 1 : 0)) * NT + tid] = neg_ln_u53((uint64_t)o[0] | ((uint64_t)o[1] << 32));
      s_c[(c1 + (c1 >= half ? 1 : 0)) * NT + tid] = neg_ln_u53((uint64_t)o[2] | ((uint64_t)o[3] << 32));
    }
    philox4x32_10((uint32_t)t, (uint32_t)(t >> 32), kCfarMcStream, (uint32_t)half, k0, k1, o);
    const double e0 = neg_ln_u53((uint64_t)o[0] | ((uint64_t)o[1] << 32));
    double re = 0.0, im = 0.0;                                  // the noise sample sqrt(E0) exp(j theta) of the CUT (SW0)
    if (g.model == ISAC_TARGET_SW0) {
      const double u2 = (double)(((uint64_t)o[2] | ((uint64_t)o[3] << 32)) >> 11) * 0x1.0p-53;
      double sn, cs;
      sincospi(2.0 * u2, &sn, &cs);
      const double r = sqrt(e0);
      re = r * cs; im = r * sn;
    }
    for (int i = 0; i < g.n_snr; ++i) {
      double p;
      if (g.model == ISAC_TARGET_SW1) p = (1.0 + snr.s[i]) * e0;
      else { const double a = snr.root[i] + re; p = a * a + im * im; }
      *cutp = p;
      const bool det = cfar_cut<M>(cutp, NT, g.c) && active;
      const unsigned long long mask = __ballot(det);
      if (lane == i) cnt += (unsigned long long)__popcll(mask);
      if (flags && active) flags[t + g.n_trials * (unsigned long long)i] = det ? 1 : 0;
    }
  }
  if (lane < g.n_snr) atomicAdd(&s_tot[lane], cnt);             // the waves of the workgroup, in LDS
  __syncthreads();
  if (tid < g.n_snr) atomicAdd(&n_det[tid], s_tot[tid]);        // one 64-bit add per workgroup and SNR point
}

}  // namespace isac

// ================================================================= host side
using namespace isac;

// Run the statement(s) with M = the method as a compile-time constant
#define CFAR_METHOD_DISPATCH(method, ...)                                                \
  switch (method) {                                                                      \
    case ISAC_CFAR_CA: { constexpr int M = ISAC_CFAR_CA; __VA_ARGS__; } break;           \
    case ISAC_CFAR_GOCA: { constexpr int M = ISAC_CFAR_GOCA; __VA_ARGS__; } break;       \
    case ISAC_CFAR_SOCA: { constexpr int M = ISAC_CFAR_SOCA; __VA_ARGS__; } break;       \
    default: { constexpr int M = ISAC_CFAR_OS; __VA_ARGS__; } break;                     \
  }

// ---------------------------------------------------------------- ThresholdFactor 'Auto': the false-alarm probability of each method at factor alpha (exponential cells)
static double soca_sum(int n, double T) {                      // 2 sum_{k<n} C(n-1+k, k) (2+T)^-(n+k), terms by the ratio recurrence (binomials overflow)
  double t = std::pow(2.0 + T, -(double)n), s = 0.0;
  for (int k = 0; k < n; ++k) {
    s += t;
    t = t * (double)(n + k) / ((double)(k + 1) * (2.0 + T));
  }
  return 2.0 * s;
}
static double pfa_of(int method, int N, int rank, double alpha) {
  const int n = N / 2;
  const double T = alpha / n;
  switch (method) {
    case ISAC_CFAR_SOCA: return soca_sum(n, T);
    case ISAC_CFAR_GOCA: return 2.0 * std::pow(1.0 + T, -(double)n) - soca_sum(n, T);
    default: {                                                  // OS
      double p = 1.0;
      for (int i = 0; i < rank; ++i) p *= (double)(N - i) / ((double)(N - i) + alpha);
      return p;
    }
  }
}
// the checks of isac_cfar.h on method, N and rank; *why: what was wrong
static int check_method(int method, int N, int rank, const char** why) {
  if (method < ISAC_CFAR_CA || method > ISAC_CFAR_OS) { *why = "unknown CFAR method"; return ISAC_ERR_INVALID_ARG; }
  if (N < 1) { *why = "TrainingBandSize must be positive"; return ISAC_ERR_INVALID_ARG; }
  if (method == ISAC_CFAR_CA) return ISAC_OK;
  if (method == ISAC_CFAR_OS && (rank < 1 || rank > N)) { *why = "OS rank must lie in 1..N"; return ISAC_ERR_INVALID_ARG; }
  if (method != ISAC_CFAR_OS && (N & 1)) { *why = "GOCA / SOCA need an even number of training cells"; return ISAC_ERR_INVALID_ARG; }
  if (N > ISAC_CFAR_MAX_TRAIN) { *why = "GOCA / SOCA / OS: more than ISAC_CFAR_MAX_TRAIN training cells"; return ISAC_ERR_UNSUPPORTED; }
  return ISAC_OK;
}
// ... and the 'Auto' factor of a method that passed them
static int threshold_factor(int method, int N, int rank, double pfa, double* alpha, const char** why) {
  const int st = check_method(method, N, rank, why);
  if (st != ISAC_OK) return st;
  if (!(pfa > 0.0 && pfa < 1.0)) { *why = "ProbabilityFalseAlarm must lie in (0, 1)"; return ISAC_ERR_INVALID_ARG; }
  if (method == ISAC_CFAR_CA) { *alpha = cfar_alpha(N, pfa); return ISAC_OK; }
  // the left sides fall strictly with alpha from 1 at alpha = 0: double the bracket until it holds the root, halve it until its ends are adjacent doubles
  double lo = 0.0, hi = 1.0;
  for (int it = 0; it < 1100 && pfa_of(method, N, rank, hi) > pfa; ++it) { lo = hi; hi *= 2.0; }
  for (int it = 0; it < 200; ++it) {
    const double mid = lo + (hi - lo) / 2.0;
    if (!(mid > lo && mid < hi)) break;
    if (pfa_of(method, N, rank, mid) > pfa) lo = mid;
    else hi = mid;
  }
  *alpha = hi;
  return ISAC_OK;
}

extern "C" int isac_cfar_threshold_factor(int32_t method, int32_t n_train, int32_t rank, double pfa, double* alpha) {
  if (!alpha) return ISAC_ERR_INVALID_ARG;
  const char* why = "";
  return threshold_factor(method, n_train, rank, pfa, alpha, &why);
}

// guard / training sizes + the method block -> the per-CUT geometry with its factor
static int cut_geom(isac_ctx* ctx, const int32_t guard[2], const int32_t train[2], double pfa, const isac_cfar_method* m, CutGeom* out) {
  if (guard[0] < 0 || guard[1] < 0 || train[0] < 0 || train[1] < 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "negative guard / training band size");
  CutGeom g{};
  g.gr = guard[0]; g.gc = guard[1];
  g.hr = guard[0] + train[0]; g.hc = guard[1] + train[1];
  const long long n_train = (2ll * g.hr + 1) * (2ll * g.hc + 1) - (2ll * g.gr + 1) * (2ll * g.gc + 1);
  if (n_train <= 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "TrainingBandSize must be positive");
  if (n_train > (1ll << 30)) return fail(ctx, ISAC_ERR_UNSUPPORTED, "training band too large");
  g.n_train = (int)n_train;
  g.rank = m->rank;
  const char* why = "";
  int st;
  if (m->custom_factor == 0.0) st = threshold_factor(m->method, g.n_train, m->rank, pfa, &g.alpha, &why);                  // 'Auto'
  else if (m->custom_factor > 0.0) { st = check_method(m->method, g.n_train, m->rank, &why); g.alpha = m->custom_factor; }   // 'Custom': pfa is not used
  else return fail(ctx, ISAC_ERR_INVALID_ARG, "custom_factor must be 0 ('Auto') or positive");                              // negative or NaN
  if (st != ISAC_OK) return fail(ctx, st, why);
  *out = g;
  return ISAC_OK;
}

extern "C" int isac_cfar2d(isac_ctx* ctx, const double* P, int32_t n_rows, int32_t n_cols, const int32_t* cut_idx, int32_t n_cut, const int32_t guard[2],
                           const int32_t train[2], double pfa, const isac_cfar_method* m, int32_t* det_idx, int32_t cap, int32_t* n_det) {
  ISAC_ENTER(ctx);
  if (!P || !cut_idx || !guard || !train || !m || !n_det || n_rows <= 0 || n_cols <= 0 || n_cut < 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "bad arguments");
  CutGeom g;
  ISAC_TRY(cut_geom(ctx, guard, train, pfa, m, &g));
  for (int i = 0; i < n_cut; ++i) {
    const int r = cut_idx[2 * i] - 1, c = cut_idx[2 * i + 1] - 1;
    if (r - g.hr < 0 || r + g.hr >= n_rows || c - g.hc < 0 || c + g.hc >= n_cols)
      return fail(ctx, ISAC_ERR_CFAR_WINDOW, "CUT training window exceeds the input matrix");
  }
  *n_det = 0;
  if (n_cut == 0) return ISAC_OK;
  const size_t pb = sizeof(double) * (size_t)n_rows * n_cols, cb = sizeof(int) * 2 * (size_t)n_cut;
  ISAC_TRY(ensure(ctx, ctx->stage_a, pb));
  ISAC_TRY(ensure(ctx, ctx->stage_b, cb));
  ISAC_TRY(ensure(ctx, ctx->stage_c, (size_t)n_cut));
  ISAC_TRY(copy_h2d(ctx, ctx->stage_a.p, P, pb));
  ISAC_TRY(copy_h2d(ctx, ctx->stage_b.p, cut_idx, cb));
  CFAR_METHOD_DISPATCH(m->method, hipLaunchKernelGGL(cfar_method_list_kernel<M>, dim3(cdiv(n_cut, 256)), dim3(256), 0, ctx->stream, (const double*)ctx->stage_a.p,
                                                     n_rows, (const int*)ctx->stage_b.p, n_cut, g, (unsigned char*)ctx->stage_c.p));
  ISAC_HIP(hipGetLastError());
  std::vector<unsigned char> flags((size_t)n_cut);
  ISAC_TRY(copy_d2h(ctx, flags.data(), ctx->stage_c.p, (size_t)n_cut));
  int n = 0;
  for (int i = 0; i < n_cut; ++i)
    if (flags[i]) {
      if (n < cap && det_idx) {
        det_idx[2 * n] = cut_idx[2 * i];
        det_idx[2 * n + 1] = cut_idx[2 * i + 1];
      }
      ++n;
    }
  *n_det = n;
  if (n > cap) return fail(ctx, ISAC_ERR_CAPACITY, "more detections than det_idx capacity");
  return ISAC_OK;
}

// The device half of isac_fft2d_redetect, on any planes [nr x nc x n_planes] with the geometry of the CPI's power window: detector m with the CPI's stored guard / training
// bands and pfa on every plane over the stored CUT rectangle, the flags compacted into per-plane CUT-order lists.  Everything stays in `scratch` (described by *pl); the
// counts and offsets are on the host when it returns.  who: the entry point, for the messages.
// K1 alone: the flags [n_planes][n_cut] (CUT order) of the CUT rows [cut_row_lo, cut_row_hi) of every plane into d_flags (sized by the caller: n_planes n_cut bytes); the
// flags of every other CUT row keep what they hold.  A flag is a function of the bits of its own guard + training window and of nothing else, so a band of rows evaluated
// again after the planes changed inside it gives the flags a run over every row would.  An empty range checks the method block and the limits and launches nothing.
int cfar_flag_planes(isac_ctx* ctx, const char* who, const isac_cfar_method* m, const double* d_planes, int n_planes, int cut_row_lo, int cut_row_hi, unsigned char* d_flags) {
  const Fft2dCpi& ts = ctx->tgt;
  const isac_cfar_config& cf = ts.cfar;
  WinGeom g{};
  ISAC_TRY(cut_geom(ctx, cf.guard, cf.train, cf.pfa, m, &g.c));
  g.nr = ts.win.nr; g.nc = ts.win.nc; g.n_cut_rows = ts.win.n_cut_rows; g.n_cut_cols = ts.win.n_cut_cols;   // (both >= 1: the submit that left the window refuses an empty zone)
  g.cut_row_lo = std::max(cut_row_lo, 0); g.cut_row_hi = std::min(cut_row_hi, g.n_cut_rows);
  if (ts.win.n_cut() * n_planes > (1ll << 30)) return fail(ctx, ISAC_ERR_UNSUPPORTED, std::string(who) + ": more than 2^30 (CUT, plane) pairs");
  // CUT columns per workgroup: as many as fit ~128 KB of LDS with the panel's kPanelRows + 2 hr rows, at most one per wave quarter (kPanelColsMax)
  const size_t budget = 128 * 1024;
  const long long fit = (long long)(budget / (sizeof(double) * (size_t)(kPanelRows + 2 * g.c.hr))) - 2ll * g.c.hc;
  if (fit < 1) return fail(ctx, ISAC_ERR_UNSUPPORTED, std::string(who) + ": guard + training band too large for the LDS-staged detector");
  g.pc = (int)std::min<long long>(fit, std::min(kPanelColsMax, g.n_cut_cols));
  const size_t lds = sizeof(double) * (size_t)(kPanelRows + 2 * g.c.hr) * (size_t)(g.pc + 2 * g.c.hc);
  if (g.cut_row_hi <= g.cut_row_lo) return ISAC_OK;
  CFAR_METHOD_DISPATCH(m->method, {
    auto kern = cfar_method_window_kernel<M>;
    ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(kern), lds));
    hipLaunchKernelGGL(kern, dim3(cdiv(g.cut_row_hi - g.cut_row_lo, kPanelRows), cdiv(g.n_cut_cols, g.pc), n_planes), dim3(kPanelRows * kPanelColsMax), lds, ctx->stream,
                       d_planes, g, d_flags);
  });
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}

int cfar_detect_planes(isac_ctx* ctx, const char* who, const isac_cfar_method* m, const double* d_planes, int n_planes, DevBuf& scratch, PlaneLists* pl) {
  const Fft2dCpi& ts = ctx->tgt;
  const CutWindow& g = ts.win;
  const long long n_cut_ll = g.n_cut();
  ISAC_TRY(cfar_flag_planes(ctx, who, m, d_planes, n_planes, 0, 0, nullptr));   // the method block and the limits, before the scratch is sized
  const int n_cut = (int)n_cut_ll;
  // every list sized for all CUTs: [det_pow n_planes n_cut | det_cut n_planes n_cut | det_cnt n_planes | row_seen n_cut_rows | flags n_planes n_cut]
  const size_t n_pairs = (size_t)n_planes * n_cut;
  const size_t off_cut = sizeof(double) * n_pairs, off_cnt = off_cut + sizeof(int) * n_pairs, off_rows = off_cnt + sizeof(int) * (size_t)n_planes;
  const size_t off_flags = off_rows + sizeof(unsigned) * (size_t)g.n_cut_rows;
  ISAC_TRY(ensure(ctx, scratch, off_flags + n_pairs));
  char* d = (char*)scratch.p;
  ISAC_HIP(hipMemsetAsync(d + off_rows, 0, sizeof(unsigned) * (size_t)g.n_cut_rows, ctx->stream));
  ISAC_TRY(cfar_flag_planes(ctx, who, m, d_planes, n_planes, 0, g.n_cut_rows, (unsigned char*)(d + off_flags)));
  hipLaunchKernelGGL(cfar_compact_kernel, dim3(n_planes), dim3(256), 0, ctx->stream, (const unsigned char*)(d + off_flags), d_planes, g.nr, g.nc, g.hr, g.hc,
                     g.n_cut_rows, n_cut, (int*)(d + off_cut), (double*)d, (int*)(d + off_cnt), (unsigned*)(d + off_rows));
  ISAC_HIP(hipGetLastError());
  std::vector<int> tail((size_t)n_planes + g.n_cut_rows);       // [det_cnt | row_seen]
  ISAC_TRY(copy_d2h(ctx, tail.data(), d + off_cnt, sizeof(int) * tail.size()));
  pl->off.assign((size_t)n_planes + 1, 0);
  long long total_ll = 0;
  for (int a = 0; a < n_planes; ++a) {
    if (tail[(size_t)a] < 0 || tail[(size_t)a] > n_cut) return fail(ctx, ISAC_ERR_HIP, "internal: detection count outside 0..nCUT");
    total_ll += tail[(size_t)a];
    pl->off[(size_t)a + 1] = (int)total_ll;
  }
  pl->rows_seen = 0;
  for (int r = 0; r < g.n_cut_rows; ++r) pl->rows_seen += tail[(size_t)n_planes + r] ? 1 : 0;
  pl->n_planes = n_planes; pl->n_cut = n_cut;
  pl->d_pow = (const double*)d; pl->d_cut = (const int*)(d + off_cut); pl->d_cnt = (const int*)(d + off_cnt);
  return ISAC_OK;
}

// ... and its lists on the host, plane after plane: cut [total] CUT ordinals, pw [total] the CUTs' powers
int cfar_fetch_lists(isac_ctx* ctx, const PlaneLists& pl, std::vector<int>& cut, std::vector<double>& pw) {
  cut.resize((size_t)pl.total());
  pw.resize((size_t)pl.total());
  for (int a = 0; a < pl.n_planes; ++a) {
    const size_t b = (size_t)pl.off[(size_t)a], n = (size_t)(pl.off[(size_t)a + 1] - pl.off[(size_t)a]);
    if (!n) continue;
    ISAC_TRY(copy_d2h(ctx, cut.data() + b, pl.d_cut + (size_t)a * pl.n_cut, sizeof(int) * n));
    ISAC_TRY(copy_d2h(ctx, pw.data() + b, pl.d_pow + (size_t)a * pl.n_cut, sizeof(double) * n));
  }
  return ISAC_OK;
}

extern "C" int isac_fft2d_redetect(isac_ctx* ctx, const isac_cfar_method* m, isac_est_result* out, int32_t* det_idx, double* det_pow, int32_t cap,
                                   int32_t* ant_offsets, int32_t* n_total) {
  ISAC_ENTER(ctx);
  if (!m || !out || cap < 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "bad arguments");
  const Fft2dCpi& ts = ctx->tgt;
  if (!ctx->last.valid || ts.state != Fft2dCpi::kCollected)
    return fail(ctx, ISAC_ERR_INVALID_ARG, "isac_fft2d_redetect: no completed fft2D on this context whose power window is still on the device");
  const int A = ts.A;
  PlaneLists pl;
  ISAC_TRY(cfar_detect_planes(ctx, "isac_fft2d_redetect", m, (const double*)ctx->pwin.p, A, ctx->redet, &pl));
  std::memset(out, 0, sizeof(*out));
  if (n_total) *n_total = pl.total();
  if (ant_offsets) std::copy(pl.off.begin(), pl.off.end(), ant_offsets);
  if (pl.total() > cap) return fail(ctx, ISAC_ERR_CAPACITY, "detection list larger than capacity");
  std::vector<int> cut;
  std::vector<double> pw;
  ISAC_TRY(cfar_fetch_lists(ctx, pl, cut, pw));
  std::vector<int32_t> det_rc;
  ISAC_TRY(fft2d_estimates(ctx, &ts.ep, ts.win, A, pl.off.data(), cut, pw, pl.rows_seen, det_rc, out));   // fft2D.m:63-99; n_azi stays 0
  if (det_idx) std::copy(det_rc.begin(), det_rc.end(), det_idx);
  if (det_pow) std::copy(pw.begin(), pw.end(), det_pow);
  return ISAC_OK;
}

extern "C" int isac_cfar_monte_carlo(isac_ctx* ctx, const isac_cfar_method* m, int32_t n_train, double pfa, int32_t target_model, const double* snr_db, int32_t n_snr,
                                     uint64_t n_trials, uint64_t seed, uint64_t* n_det, uint8_t* flags) {
  ISAC_ENTER(ctx);
  if (!m || !snr_db || !n_det) return fail(ctx, ISAC_ERR_INVALID_ARG, "bad arguments");
  if (n_train < 2 || (n_train & 1)) return fail(ctx, ISAC_ERR_INVALID_ARG, "isac_cfar_monte_carlo: n_train must be even and at least 2");
  if (n_train > ISAC_CFAR_MC_MAX_TRAIN) return fail(ctx, ISAC_ERR_UNSUPPORTED, "isac_cfar_monte_carlo: more than ISAC_CFAR_MC_MAX_TRAIN training cells");
  if (target_model != ISAC_TARGET_SW0 && target_model != ISAC_TARGET_SW1) return fail(ctx, ISAC_ERR_INVALID_ARG, "isac_cfar_monte_carlo: unknown target model");
  if (n_snr < 1 || n_snr > kMcMaxSnr) return fail(ctx, ISAC_ERR_INVALID_ARG, "isac_cfar_monte_carlo: n_snr must lie in 1..64");
  if (n_trials < 1 || n_trials > (1ull << 40)) return fail(ctx, ISAC_ERR_INVALID_ARG, "isac_cfar_monte_carlo: n_trials must lie in 1..2^40");
  if (flags && n_trials > (1ull << 22)) return fail(ctx, ISAC_ERR_INVALID_ARG, "isac_cfar_monte_carlo: per-trial flags need n_trials <= 2^22");
  McGeom g{};
  McSnr snr{};
  for (int i = 0; i < n_snr; ++i) {
    if (snr_db[i] != snr_db[i] || snr_db[i] == HUGE_VAL) return fail(ctx, ISAC_ERR_INVALID_ARG, "isac_cfar_monte_carlo: snr_db must be finite or -inf");
    snr.s[i] = std::pow(10.0, snr_db[i] / 10.0);                // -inf: 0, the false-alarm point
    snr.root[i] = std::sqrt(snr.s[i]);
  }
  const int32_t guard[2] = {0, 0}, train[2] = {0, n_train / 2}; // the 1 x (N + 1) window: N/2 columns on either side of the CUT
  ISAC_TRY(cut_geom(ctx, guard, train, pfa, m, &g.c));
  g.n_snr = n_snr; g.model = target_model; g.n_trials = n_trials; g.seed = seed;
  // 256 lanes while the tile of N + 1 cells per lane fits ~128 KB of LDS (N <= 62), 128 lanes beyond (N = 128: 129 KB of the CU's 160)
  const int nt = sizeof(double) * (size_t)(n_train + 1) * 256 <= 128 * 1024 ? 256 : 128;
  const size_t lds = sizeof(double) * (size_t)(n_train + 1) * (size_t)nt;
  const int per_cu = (int)std::max<size_t>(1, std::min<size_t>((160 * 1024) / (lds + 1024), 2048 / nt));   // resident workgroups per CU: LDS, 32 waves
  const size_t off_flags = sizeof(unsigned long long) * kMcMaxSnr, flag_bytes = flags ? (size_t)n_trials * (size_t)n_snr : 0;
  ISAC_TRY(ensure(ctx, ctx->cfar_mc, off_flags + flag_bytes));
  char* d = (char*)ctx->cfar_mc.p;
  ISAC_HIP(hipMemsetAsync(d, 0, off_flags, ctx->stream));
  for (unsigned long long t0 = 0; t0 < n_trials; t0 += kMcLaunchTrials) {
    g.t0 = t0;
    g.n = std::min<unsigned long long>(kMcLaunchTrials, n_trials - t0);
    const unsigned grid = (unsigned)std::min<unsigned long long>((g.n + nt - 1) / nt, 256ull * per_cu * 2);   // two waves of workgroups over 256 CUs; grid-stride loop
    CFAR_METHOD_DISPATCH(m->method, {
      auto kern = nt == 256 ? cfar_mc_kernel<M, 256> : cfar_mc_kernel<M, 128>;
      ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(kern), lds));
      hipLaunchKernelGGL(kern, dim3(grid), dim3(nt), lds, ctx->stream, g, snr, (unsigned long long*)d, flags ? (unsigned char*)(d + off_flags) : (unsigned char*)nullptr);
    });
    ISAC_HIP(hipGetLastError());
  }
  static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "n_det is copied out as it is counted");
  ISAC_TRY(copy_d2h(ctx, n_det, d, sizeof(uint64_t) * (size_t)n_snr));
  if (flags) ISAC_TRY(copy_d2h(ctx, flags, d + off_flags, flag_bytes));
  return ISAC_OK;
}
