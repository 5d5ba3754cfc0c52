// MUSIC (gfx950): the signal-subspace kernel, the angle scan and the music2D kernels.  The eigensolver in front of them: eigh.hip; the array covariance: cov.hip.
// Reference path: fft2D.m:106-111 -> doaEstimation.music (+sensing/+estimation/+doaEstimation/music.m).
//   [Ua,Sa] = eig(Ra); descending sort; Uan = Ua(:,L+1:end); P(phi) = 1/(a' Uan Uan' a + eps)
#include "isac_internal.hpp"
#include "eigh_dev.hpp"

namespace isac {

// ---------------------------------------------------------------- the SIGNAL SUBSPACE only (music.m:19-29; "Hermitian eigensolver III" of eigh.hip)
//   K1, K2  eigh_tridiag_*, eigh_bisect_kernel: the Householder reflectors (S.M, S.tau), the real tridiagonal (S.d, S.e) and ALL eigenvalues -- eigh.hip
//   K3  music_subspace_kernel    after numDets is known (CFAR branch): block inverse iteration on T for the L largest eigenvalues -- one lane
//                                per vector, Gaussian elimination with partial pivoting (dlagtf / dlagts), two rounds from pseudo-random
//                                start vectors with modified Gram-Schmidt in descending-eigenvalue order in between (exactly degenerate
//                                clusters end up with an orthonormal basis of their eigenspace, like dstein) -- then U = Q Z through the
//                                reflectors, one wavefront per vector
//   K4  music_scan_kernel        a' Uan Uan' a = || a - Us Us' a ||^2  (a sum of squares: no cancellation at the peaks)
// L >= A (empty noise space) and L <= 0 need no vectors; L beyond the LDS capacity of K3 falls back to the QL pipeline, whose kernels are
// always enqueued behind K3 and return at once when K3 reports success in `ctl` (numDets lives on the device: no host decision).

// K3.  LDS: SubspaceLds (lane v owns column v of its planes: consecutive lanes touch consecutive doubles).  R = rows per lane in the
// wave-per-vector phases (n <= 64 R).
template <int R>
__global__ __launch_bounds__(1024) void music_subspace_kernel(int n, void* scratch, const int* __restrict__ num_dets_dev, int num_dets_host,
                                                              int lmax, int lv, c64* __restrict__ U_out /* [n x L] */, int* __restrict__ ctl,
                                                              EighInfo* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  __shared__ int s_bad;
  __shared__ double s_red[16];
  EighScratch S(scratch, n);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int L = num_dets_dev ? *num_dets_dev : num_dets_host;        // music.m:21-25
  if (L <= 0 || L >= n || L > lmax) {                                // (uniform) nothing to compute / beyond this kernel's capacity
    if (tid == 0) {
      const bool done = L <= 0 || L >= n;
      ctl[MusicCtl::kRoute] = done ? 1 : 0;
      ctl[MusicCtl::kLsub] = L <= 0 ? 0 : L;
      if (done && info) { eigh_set_status(info, 0); info->rotations = kEighRouteSubspace; }
    }
    return;
  }
  const long long t_k0 = clock64();
  long long t_solve = 0, t_mgs = 0;                                  // phase instrumentation (ISAC_DEBUG): cycles of thread 0
  const SubspaceLds lds = SubspaceLds::of(n, lv);
  double* u0 = reinterpret_cast<double*>(smem_raw + lds.u0);         // 1 / pivot
  double* u1 = reinterpret_cast<double*>(smem_raw + lds.u1);
  double* u2 = reinterpret_cast<double*>(smem_raw + lds.u2);
  double* y = reinterpret_cast<double*>(smem_raw + lds.y);           // right-hand sides / solutions = the vectors, [row][vector]
  double* sd = reinterpret_cast<double*>(smem_raw + lds.sd);         // d
  double* se = reinterpret_cast<double*>(smem_raw + lds.se);         // e (e[n-1] = 0)
  c64* s_tau = reinterpret_cast<c64*>(smem_raw + lds.tau);           // reflector scalars
  double tn = 0.0;
  for (int i = tid; i < n; i += 1024) {
    const double d = S.d[i], e = i < n - 1 ? S.e[i] : 0.0;
    sd[i] = d; se[i] = e;
    s_tau[i] = i < n - 1 ? S.tau[i] : mk(0.0, 0.0);
    tn = fmax(tn, fmax(fabs(d), fabs(e)));
  }
  tn = wave_max(tn);
  if (tid == 0) s_bad = 0;
  if (lane == 0) s_red[wid] = tn;
  __syncthreads();
  tn = 0.0;
  for (int w = 0; w < 16; ++w) tn = fmax(tn, s_red[w]);
  // pivot floor of the elimination: eps ||T||.  The matrix is safe-scaled (entries inside [2^-400, 2^400], or exactly zero): the 2^-400
  // floor keeps 1 / tiny and the squared norms of the solutions finite for the zero matrix too (any orthonormal basis is right there)
  const double tiny = 2.220446049250313e-16 * fmax(tn, 0x1.0p-400);
  const bool solver = wid == 0 && lane < L;                          // one lane per vector, descending eigenvalue order
  const double lam = solver ? S.wsc[n - 1 - lane] : 0.0;
  if (solver) {                                                      // deterministic pseudo-random start vectors (same LCG as the restatement)
    unsigned s = 0x9E3779B9u * (unsigned)(lane + 1) + 0x7F4A7C15u;
    for (int i = 0; i < n; ++i) {
      s = 1664525u * s + 1013904223u;
      y[(size_t)i * lv + lane] = (double)(s >> 8) * (1.0 / 16777216.0) - 0.5;
    }
  }
  __syncthreads();
  const long long t_k1 = clock64();
  // Two rounds: with eigenvalues good to 2 eps ||T|| the first solve already leaves an error of ~1e-14, the second reaches working precision
  // (oracle/subspace_music.py, ROUNDS: orthonormality and invariant-subspace residuals at 1e-16 after two rounds on every test spectrum,
  // the exactly degenerate ones included -- dstein's own loop typically stops after two or three)
  constexpr int kRounds = 2;
  for (int round = 0; round < kRounds; ++round) {
    const long long t_r0 = clock64();
    if (solver) {
      // ---- (T - lam I) y = x : elimination with row interchanges; the forward substitution rides along.  A lone wavefront pays every
      // LDS round trip in full, so the operands of step i + 1 are fetched before the dependent arithmetic of step i (they do not depend on it).
      double a = sd[0] - lam, b = se[0];
      double ycur = y[lane];
      double c_n = se[0], dn_n = sd[1] - lam, en_n = se[1], yn_n = y[(size_t)lv + lane];
      for (int i = 0; i < n - 1; ++i) {
        const double c = c_n, dn = dn_n, en = en_n, ynext = yn_n;
        {
          const int i1 = i + 1 < n - 1 ? i + 1 : i;                  // (clamped: the last trip's prefetch is unused)
          c_n = se[i1]; dn_n = sd[i1 + 1] - lam; en_n = se[i1 + 1]; yn_n = y[(size_t)(i1 + 1) * lv + lane];
        }
        const bool swap = fabs(a) < fabs(c);
        double piv = swap ? c : a;
        piv = fabs(piv) < tiny ? (piv < 0.0 ? -tiny : tiny) : piv;   // singular to working precision: dlagts' pivot perturbation (also keeps 1 / piv finite)
        const double inv = rcp_fast(piv);
        const double m = (swap ? a : c) * inv;
        const size_t o = (size_t)i * lv + lane;
        u0[o] = inv;
        u1[o] = swap ? dn : b;
        u2[o] = swap ? en : 0.0;
        const double an = swap ? ::fma(-m, dn, b) : ::fma(-m, b, dn);
        b = swap ? -m * en : en;
        a = an;
        const double yi = swap ? ynext : ycur, yo = swap ? ycur : ynext;
        y[o] = yi;
        ycur = ::fma(-m, yi, yo);
      }
      if (fabs(a) < tiny) a = a < 0.0 ? -tiny : tiny;
      {
        const size_t o = (size_t)(n - 1) * lv + lane;
        u0[o] = rcp_fast(a); u1[o] = 0.0; u2[o] = 0.0;
        y[o] = ycur;
      }
      double y1 = 0.0, y2 = 0.0;
      {
        size_t o = (size_t)(n - 1) * lv + lane;
        double p0 = u0[o], p1 = u1[o], p2 = u2[o], py = y[o];
        for (int i = n - 1; i >= 0; --i) {
          const double q0 = p0, q1 = p1, q2 = p2, qy = py;
          const size_t oc = o;
          if (i > 0) { o -= lv; p0 = u0[o]; p1 = u1[o]; p2 = u2[o]; py = y[o]; }   // operands of the next step, under this step's arithmetic
          const double v = ::fma(-q2, y2, ::fma(-q1, y1, qy)) * q0;
          y[oc] = v;
          y2 = y1; y1 = v;
        }
      }
    }
    __syncthreads();
    const long long t_r1 = clock64();
    t_solve += t_r1 - t_r0;
    if (wid == 0) {
      // ---- modified Gram-Schmidt, descending-eigenvalue order (lanes = rows); twice after the last round
      const int passes = round == kRounds - 1 ? 2 : 1;
      for (int p = 0; p < passes; ++p)
        for (int j = 0; j < L; ++j) {
          double zj[R];
#pragma unroll
          for (int r = 0; r < R; ++r) { const int i = lane + 64 * r; zj[r] = i < n ? y[(size_t)i * lv + j] : 0.0; }
          for (int i2 = 0; i2 < j; ++i2) {
            double zi[R], dot = 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r) { const int i = lane + 64 * r; zi[r] = i < n ? y[(size_t)i * lv + i2] : 0.0; dot = ::fma(zi[r], zj[r], dot); }
            dot = wave_sum_dpp(dot);
#pragma unroll
            for (int r = 0; r < R; ++r) zj[r] = ::fma(-dot, zi[r], zj[r]);
          }
          double nrm = 0.0;
#pragma unroll
          for (int r = 0; r < R; ++r) nrm = ::fma(zj[r], zj[r], nrm);
          nrm = wave_sum_dpp(nrm);
          const bool ok = nrm > 0.0 && nrm < 1.7976931348623157e308;
          const double inv = ok ? 1.0 / sqrt(nrm) : 0.0;
          if (!ok && lane == 0) s_bad = 1;
#pragma unroll
          for (int r = 0; r < R; ++r) { const int i = lane + 64 * r; if (i < n) y[(size_t)i * lv + j] = zj[r] * inv; }
        }
    }
    __syncthreads();
    t_mgs += clock64() - t_r1;
  }
  const long long t_k2 = clock64();
  // ---- U = Q Z, Q = H_0 ... H_{n-2} (zungtr's product, applied to L vectors instead of formed): one wavefront per vector (two when
  // L > 16).  The reflectors come through LDS in chunks of 16 columns fetched by the whole workgroup (the dead elimination planes; the
  // next chunk's global loads fly under the current chunk's arithmetic): a wavefront that fetched its own columns from L2 step by step
  // waited a round trip per reflector (85 us at n = 64, most of it here).
  constexpr int CH = 16;
  const c64* M = S.M;
  c64* s_ref = reinterpret_cast<c64*>(u0);                           // [CH][n]  (3 n lv doubles >= 16 n complex for every supported n)
  const int n_chunks = (n - 1 + CH - 1) / CH;
  c64 pre[R];
  auto fetch_chunk = [&](int c) {
    const int k_hi = n - 2 - CH * c;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int e = tid + 1024 * r;                                  // (kl, i) = (e / n, e % n); CH n = 1024 R elements exactly when n = 64 R
      const int kl = e / n, i = e - kl * n;
      const int k = k_hi - kl;
      const bool in = kl < CH && k >= 0;
      const c64 raw = M[(size_t)i + (size_t)n * (in ? k : 0)];       // (unconditional, clamped)
      pre[r] = !in ? mk(0.0, 0.0) : (i > k + 1 ? raw : mk(i == k + 1 ? 1.0 : 0.0, 0.0));
    }
  };
  c64 u[2][R];
  const bool has0 = wid < L, has1 = R <= 2 && wid + 16 < L;          // (orders above 128: at most 16 vectors, one per wavefront -- host side)
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = lane + 64 * r;
    u[0][r] = mk((has0 && i < n) ? y[(size_t)i * lv + wid] : 0.0, 0.0);
    u[1][r] = mk((has1 && i < n) ? y[(size_t)i * lv + wid + 16] : 0.0, 0.0);
  }
  fetch_chunk(0);
  __syncthreads();                                                   // the vectors are in registers: the planes are free
  for (int c = 0; c < n_chunks; ++c) {
#pragma unroll
    for (int r = 0; r < R; ++r) { const int e = tid + 1024 * r; if (e < CH * n) s_ref[e] = pre[r]; }
    __syncthreads();
    if (c + 1 < n_chunks) fetch_chunk(c + 1);
    const int k_hi = n - 2 - CH * c;
    if (has0) {                                                      // (wave-uniform)
#pragma unroll
      for (int kl = 0; kl < CH; ++kl) {
        const int k = k_hi - kl;
        if (k < 0) break;
        const c64 tau = s_tau[k];
        c64 vk[R], s0 = mk(0.0, 0.0), s1 = mk(0.0, 0.0);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int i = lane + 64 * r;
          vk[r] = i < n ? s_ref[kl * n + i] : mk(0.0, 0.0);
          s0 = fma(conj(vk[r]), u[0][r], s0);
          if (has1) s1 = fma(conj(vk[r]), u[1][r], s1);
        }
        s0.re = wave_sum_dpp(s0.re); s0.im = wave_sum_dpp(s0.im);
        const c64 t0 = tau * s0;
#pragma unroll
        for (int r = 0; r < R; ++r) u[0][r] = u[0][r] - t0 * vk[r];
        if (has1) {
          s1.re = wave_sum_dpp(s1.re); s1.im = wave_sum_dpp(s1.im);
          const c64 t1 = tau * s1;
#pragma unroll
          for (int r = 0; r < R; ++r) u[1][r] = u[1][r] - t1 * vk[r];
        }
      }
    }
    __syncthreads();
  }
  bool bad = false;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int i = lane + 64 * r;
    if (i < n) {
      if (has0) { U_out[(size_t)i + (size_t)n * wid] = u[0][r]; bad = bad || !(fabs(u[0][r].re) <= 2.0 && fabs(u[0][r].im) <= 2.0); }   // unit vectors; catches NaN / Inf input
      if (has1) { U_out[(size_t)i + (size_t)n * (wid + 16)] = u[1][r]; bad = bad || !(fabs(u[1][r].re) <= 2.0 && fabs(u[1][r].im) <= 2.0); }
    }
  }
  if (__any(bad) && lane == 0) s_bad = 1;
  __syncthreads();
  if (tid == 0) {                                  // (no fence: the consumers are later kernels of the same stream)
    ctl[MusicCtl::kRoute] = 1;
    ctl[MusicCtl::kLsub] = L;
    if (info) {
      eigh_set_status(info, s_bad ? kEighNotFinite : 0); info->rotations = kEighRouteSubspace;
      info->sub_setup = (int)((t_k1 - t_k0) >> 6); info->sub_solve = (int)(t_solve >> 6); info->sub_mgs = (int)(t_mgs >> 6); info->sub_back = (int)((clock64() - t_k2) >> 6);
    }
  }
}

// ---------------------------------------------------------------- MUSIC pseudo-spectrum (ULA), music.m:82-91
// One workgroup per scan angle.  Noise subspace = eigenvectors whose descending rank >= L.
// mode 0: MUSIC  1/(a' Uan Uan' a + eps);  mode 1: digital beamforming |a' Ra a| (digitalBF.m:72);
// mode 2: MVDR 1/(a' Ra^-1 a + eps) (mvdrBF.m:72) -- all three are weighted sums of |v_i' a|^2 over the eigenpairs.
__global__ __launch_bounds__(256) void music_scan_kernel(const double* __restrict__ w, const c64* __restrict__ V, int A,
                                                         const int* __restrict__ num_dets_dev, int num_dets_host,
                                                         const double* __restrict__ sind_tab, double d_ratio, double eps1,
                                                         double* __restrict__ p_out, int mode, const int* __restrict__ ctl) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  c64* s_a = reinterpret_cast<c64*>(smem_raw);     // steering vector [A]
  c64* s_c = s_a + A;                              // [<= 32] u_s' a (subspace route)
  __shared__ double s_red[4];
  const int tid = threadIdx.x;
  const int Lsig = num_dets_dev ? *num_dets_dev : num_dets_host;
  const double sd = sind_tab[blockIdx.x];
  for (int m = tid; m < A; m += blockDim.x) {
    // exp(-2j*pi*m*d*sind(ph)) evaluated left to right like the reference expression (music.m:82)
    double arg = ((-2.0 * M_PI) * (double)m) * d_ratio;
    arg = arg * sd;
    double s, c;
    sincos(arg, &s, &c);
    s_a[m] = mk(c, s);
  }
  __syncthreads();
  double acc = 0.0;
  const bool subspace = mode == 0 && ctl && ctl[MusicCtl::kRoute] == 1;       // (grid-uniform)
  if (subspace) {
    // a' Uan Uan' a = || a - Us Us' a ||^2 with the Ls signal vectors of music_subspace_kernel in V[:, 0..Ls)
    const int Ls = ctl[MusicCtl::kLsub];
    if (Ls < A) {                                  // (Ls >= A: empty noise space, the quadratic form is 0 -- music.m:28 with L >= nAnts)
      const int lane = tid & 63, wid = tid >> 6;
      for (int sv = wid; sv < Ls; sv += 4) {
        const c64* col = V + (long long)A * sv;
        c64 y = mk(0.0, 0.0);
        for (int m = lane; m < A; m += 64) y = fma(conj(col[m]), s_a[m], y);
        y.re = wave_sum(y.re); y.im = wave_sum(y.im);
        if (lane == 0) s_c[sv] = y;
      }
      __syncthreads();
      for (int m = tid; m < A; m += blockDim.x) {
        c64 r = s_a[m];
        for (int sv = 0; sv < Ls; ++sv) r = r - V[m + (long long)A * sv] * s_c[sv];
        acc = ::fma(r.re, r.re, ::fma(r.im, r.im, acc));
      }
    }
  } else {
    for (int v = tid; v < A; v += blockDim.x) {
      // descending rank of eigenvalue v (stable: ties keep index order)
      const double wv = w[v];
      double weight = 1.0;
      if (mode == 0) {
        int rank = 0;
        for (int j = 0; j < A; ++j) rank += (w[j] > wv || (w[j] == wv && j < v)) ? 1 : 0;
        if (rank < Lsig) continue;                    // signal subspace
      } else {
        weight = (mode == 1) ? wv : 1.0 / wv;
      }
      c64 y = mk(0.0, 0.0);
      const c64* col = V + (long long)A * v;
      for (int m = 0; m < A; ++m) y = fma(conj(col[m]), s_a[m], y);
      acc += weight * (y.re * y.re + y.im * y.im);
    }
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o);
  if ((tid & 63) == 0) s_red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += s_red[i];
    p_out[blockIdx.x] = (mode == 1) ? fabs(t) : fabs(1.0 / (t + eps1));    // music.m:90,94 / digitalBF.m:72,76 / mvdrBF.m:72,76
  }
}

// ---------------------------------------------------------------- music2D (music2D.m:67-108) building blocks
// H = rx(:,:,1) .* conj(tx(:,:,1))   [K x Ls]                                               music2D.m:67-68
__global__ __launch_bounds__(256) void chan_plane_kernel(const c64* __restrict__ rx, const c64* __restrict__ tx, long long n,
                                                         c64* __restrict__ h) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) h[i] = mul_conj(rx[i], tx[i]);
}

// Signal-subspace vectors of Rr = H H^H / Ls obtained from the small Gram problem (G/K) v = mu v:
//   u_i = H v_i / sqrt(K mu_i)        (unit norm; the K - Ls dimensional null space never has to be formed)
__global__ __launch_bounds__(256) void signal_vectors_kernel(const c64* __restrict__ Hc /* [K x Ls] */, int K, int Ls,
                                                             const double* __restrict__ w, const c64* __restrict__ V /* [Ls x Ls] */,
                                                             const int* __restrict__ top /* [Lsig] eigen indices */, int Lsig,
                                                             c64* __restrict__ U /* [K x Lsig] */) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = blockIdx.y;
  if (n >= K || i >= Lsig) return;
  const int e = top[i];
  const c64* v = V + (long long)Ls * e;
  c64 acc = mk(0.0, 0.0);
  for (int m = 0; m < Ls; ++m) acc = fma(Hc[n + (long long)K * m], v[m], acc);
  const double nrm = sqrt((double)K * w[e]);
  U[n + (long long)K * i] = mk(acc.re / nrm, acc.im / nrm);
}

// Sum of v over the 256 threads of the block, in every thread (s_red: 4 doubles, free again on return)
__device__ inline double music2d_block_sum(double v, double* s_red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return s_red[0] + s_red[1] + s_red[2] + s_red[3];
}

// P(x) = 1 / || a(x) - sum_i e_i (e_i^H a(x)) ||^2,  a(x)[n] = exp(j * ((coef * x) * n) / den)   (music2D.m:92-93,98-108)
// = 1 / (a^H Un Un^H a) for the orthonormal signal vectors e_i: the residual is summed term by term, so a denominator 1e-10 N (a target on the scan grid
// at 100 dB) keeps its digits; N - sum_i |e_i^H a|^2, the same number, would lose them.
// conj_u = 0: e_i = U[:, i] (range, U = Urs);  conj_u = 1: e_i = conj(U[:, cols[i]]) (velocity, Uvs = conj(V)).  Dynamic LDS: 4 + 2 Lsig doubles.
constexpr int kMusic2dChunk = 4;     // projections formed per pass over a(x)
__global__ __launch_bounds__(256) void music2d_scan_kernel(const c64* __restrict__ U, int N, int ldU, const int* __restrict__ cols,
                                                           int Lsig, int conj_u, double coef, double den, double x0, double dx,
                                                           double* __restrict__ p_out) {
  extern __shared__ __align__(16) double s_m2d[];
  double* s_red = s_m2d;
  c64* s_y = reinterpret_cast<c64*>(s_m2d + 4);      // y_i = e_i^H a(x)
  const double x = x0 + dx * (double)blockIdx.x;
  const double a = coef * x;
  for (int i0 = 0; i0 < Lsig; i0 += kMusic2dChunk) {
    const int nb = min(kMusic2dChunk, Lsig - i0);
    const c64* u[kMusic2dChunk];
    c64 y[kMusic2dChunk];
#pragma unroll
    for (int j = 0; j < kMusic2dChunk; ++j) {
      const int i = i0 + min(j, nb - 1);
      u[j] = U + (long long)ldU * (cols ? cols[i] : i);
      y[j] = mk(0.0, 0.0);
    }
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
      double s, c;
      sincos((a * (double)n) / den, &s, &c);
#pragma unroll
      for (int j = 0; j < kMusic2dChunk; ++j)
        if (j < nb) y[j] = fma(conj_u ? u[j][n] : conj(u[j][n]), mk(c, s), y[j]);
    }
#pragma unroll
    for (int j = 0; j < kMusic2dChunk; ++j) {
      if (j >= nb) break;                                        // (nb is uniform over the block)
      const double yr = music2d_block_sum(y[j].re, s_red), yi = music2d_block_sum(y[j].im, s_red);
      if (threadIdx.x == 0) s_y[i0 + j] = mk(yr, yi);
    }
  }
  __syncthreads();
  double q = 0.0;
  for (int n = threadIdx.x; n < N; n += blockDim.x) {
    double s, c;
    sincos((a * (double)n) / den, &s, &c);
    c64 r = mk(c, s);
    for (int i = 0; i < Lsig; ++i) {
      const c64 un = U[(long long)ldU * (cols ? cols[i] : i) + n];
      r = r - (conj_u ? conj(un) : un) * s_y[i];
    }
    q += r.re * r.re + r.im * r.im;
  }
  q = music2d_block_sum(q, s_red);
  if (threadIdx.x == 0) p_out[blockIdx.x] = 1.0 / q;
}

}  // namespace isac

// ================================================================= host side
using namespace isac;

// ---- MUSIC's signal-subspace route: supported orders, and the second of the two halves around the wait for numDets (the first: isac_music_tridiag_bisect_dev, eigh.hip)
static int* music_ctl(isac_ctx* ctx) { return reinterpret_cast<int*>((char*)ctx->misc.p + 256); }   // (ctx->misc: >= 512 bytes here)
bool isac_music_subspace_ok(isac_ctx* ctx, int A) {
  return ctx->music_route == 0 && A >= 3 && A <= 256;
}
// second half: the L = numDets signal vectors into ctx->eig_v[:, 0..L) (L from the device -- the CFAR branch -- or from the host), then the
// QL pipeline as the conditional fallback (L beyond the subspace kernel's capacity)
int isac_music_subspace_dev(isac_ctx* ctx, int A, const int* d_num_dets, int num_dets_host, hipStream_t st) {
  if (!st) st = ctx->stream;
  const int n = A;
  EighInfo* info = eig_info(ctx, A);
  int* ctl = music_ctl(ctx);
  const SubspaceLds lds = SubspaceLds::of(n);
#define ISAC_SUBSPACE(RR)                                                                                                         \
  do {                                                                                                                            \
    ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(music_subspace_kernel<RR>), (size_t)(150 * 1024)));                     \
    hipLaunchKernelGGL(music_subspace_kernel<RR>, dim3(1), dim3(1024), lds.bytes, st, n, ctx->eig_scratch.p, d_num_dets,          \
                       num_dets_host, lds.lmax, lds.lv, (c64*)ctx->eig_v.p, ctl, info);                                           \
  } while (0)
  if (n <= 64) ISAC_SUBSPACE(1); else if (n <= 128) ISAC_SUBSPACE(2); else ISAC_SUBSPACE(4);
#undef ISAC_SUBSPACE
  ISAC_HIP(hipGetLastError());
  return isac_eigh_ql_dev(ctx, n, st, ctl);
}
const int* isac_music_ctl(isac_ctx* ctx) { return music_ctl(ctx); }

// scan: uses ctx->eig_w / eig_v; L from device pointer (fused pipeline) or host value
int isac_music_scan_dev(isac_ctx* ctx, int A, const int* d_num_dets, int num_dets_host, const double* d_sind, int n_steps,
                        double d_ratio, double* d_spec, hipStream_t st, int mode, const int* ctl) {
  if (!st) st = ctx->stream;
  hipLaunchKernelGGL(music_scan_kernel, dim3(n_steps), dim3(256), sizeof(c64) * ((size_t)A + 32), st,
                     (const double*)ctx->eig_w.p, (const c64*)ctx->eig_v.p, A, d_num_dets, num_dets_host, d_sind, d_ratio,
                     2.220446049250313e-16, d_spec, mode, ctl);
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}

// ---- music2D stages (host side lives in doa.hip)
int isac_music2d_plane(isac_ctx* ctx, const c64* d_rx, const c64* d_tx, long long n, c64* d_h) {
  hipLaunchKernelGGL(chan_plane_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, d_rx, d_tx, n, d_h);
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}
int isac_music2d_signal_vectors(isac_ctx* ctx, const c64* d_h, int K, int Ls, const int* d_top, int Lsig, c64* d_U) {
  hipLaunchKernelGGL(signal_vectors_kernel, dim3(cdiv(K, 256), Lsig), dim3(256), 0, ctx->stream, d_h, K, Ls, (const double*)ctx->eig_w.p,
                     (const c64*)ctx->eig_v.p, d_top, Lsig, d_U);
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}
int isac_music2d_scan(isac_ctx* ctx, const c64* d_U, int N, int ldU, const int* d_cols, int Lsig, int conj_u, double coef, double den,
                      double x0, double dx, int n_steps, double* d_p) {
  hipLaunchKernelGGL(music2d_scan_kernel, dim3(n_steps), dim3(256), sizeof(double) * (4 + 2 * (size_t)Lsig), ctx->stream, d_U, N, ldU, d_cols, Lsig, conj_u, coef, den, x0, dx,
                     d_p);
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}
