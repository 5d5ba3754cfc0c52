// Hermitian eigendecomposition (gfx950): eig(Ra) of music.m:19 for isac_eigh / isac_eigh_top, DBF / MVDR, music2D and MUSIC (the scan and the
// signal-subspace kernel: music.hip).
#include <algorithm>
#include <atomic>
#include "isac_internal.hpp"
#include "eigh_dev.hpp"

namespace isac {

// zheev-style safe scaling: when the largest |entry| lies outside [2^-400, 2^400] (squares would under/overflow), the
// matrix is multiplied by an exact power of two on load and the eigenvalues by its inverse on output.  Returns the factor
// (1.0 in the normal range, so ordinary inputs are untouched bit for bit).  s_red: >= 16 doubles of LDS.
__device__ __forceinline__ double eigh_scale_of(double t /* the largest |entry| */) {
  if (!(t > 0.0) || !(t < 1.7976931348623157e308)) return 1.0;      // zero matrix, Inf or NaN: leave as is
  const int ex = ilogb(t);
  return (ex < -400 || ex > 400) ? ldexp(1.0, -ex) : 1.0;
}
__device__ __forceinline__ double eigh_safe_scale(const c64* __restrict__ Hin, int count, double* s_red) {
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wid = tid >> 6, nw = nt >> 6;
  double mx = 0.0;
  for (int i = tid; i < count; i += nt) { const c64 v = Hin[i]; mx = fmax(mx, fmax(fabs(v.re), fabs(v.im))); }
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_down(mx, o));
  __syncthreads();
  if (lane == 0) s_red[wid] = mx;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < nw; ++w) t = fmax(t, s_red[w]);
  __syncthreads();
  return eigh_scale_of(t);
}

// ---------------------------------------------------------------- Hermitian eigensolver: one-workgroup cyclic Jacobi in LDS
// Round-robin (tournament) ordering: A/2 disjoint rotations per round, A-1 rounds per sweep.
constexpr int kJacobiMaxA = 16;    // isac_eigh_dev: Jacobi up to this order, the tridiagonal pipeline beyond (the kernel's LDS carve holds up to 64)

__device__ __forceinline__ void rr_pair(int round, int k, int n /* even */, int& p, int& q) {
  // circle method: position 0 fixed, others rotate
  const int m = n - 1;
  int a = (k == 0) ? m : (round + k) % m;
  int b = (round + m - k) % m;
  if (k == 0) { a = m; b = round % m; }
  p = a < b ? a : b;
  q = a < b ? b : a;
}

// Two barriers per round:
//   P: lanes k < n/2 read the pivot 2x2 of pair k and derive the complex rotation
//        J_k = [[c, g], [-conj(g), c]],  g = s e^{j phi}      (no |beta| needed:
//        u = sign(d) 2 / (|d| + sqrt(d^2 + 4|beta|^2)),  c = 1/sqrt(1 + u^2 |beta|^2),  g = c u beta)
//   U: thread (a, b) owns the 2x2 block (pair a) x (pair b) of H and applies  J_a^H B J_b  in place
//      (a one-phase two-sided update -- nobody else touches that block this round); the same
//      threads rotate two (row, pair) column pairs of V.
// A <= 64: H and V live in LDS.  Larger arrays take the tridiagonal route below (the same algorithm on a global scratch
// was 99 ms at A = 256).
__global__ __launch_bounds__(1024) void jacobi_eigh_kernel(const c64* __restrict__ Hin, int A, int max_sweeps,
                                                           double* __restrict__ w_out, c64* __restrict__ V_out,
                                                           EighInfo* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const JacobiLds lds = JacobiLds::of(A);
  const int n = lds.n;                             // A padded to even with an isolated zero row/col
  const int h = lds.h;
  c64* H = reinterpret_cast<c64*>(smem_raw + lds.H);
  c64* V = reinterpret_cast<c64*>(smem_raw + lds.V);
  c64* rg = reinterpret_cast<c64*>(smem_raw + lds.rg);
  double* rc = reinterpret_cast<double*>(smem_raw + lds.rc);
  int* rp = reinterpret_cast<int*>(smem_raw + lds.rp);
  int* rq = reinterpret_cast<int*>(smem_raw + lds.rq);
  const int tid = threadIdx.x, nt = blockDim.x;
  const double scl = eigh_safe_scale(Hin, A * A, reinterpret_cast<double*>(smem_raw));   // (LDS not in use yet; >= 128 B for n >= 2)
  for (int i = tid; i < n * n; i += nt) {
    int r = i % n, c = i / n;
    H[i] = (r < A && c < A) ? Hin[r + (long long)A * c] * scl : mk(0.0, 0.0);
    V[i] = mk(r == c ? 1.0 : 0.0, 0.0);
  }
  __syncthreads();
  // Convergence: a sweep in which every pivot satisfied |h_pq|^2 <= tol^2 |h_pp h_qq| (relative to the
  // diagonal pair, Demmel-Veselic style -- keeps the tiny noise eigen-pairs accurate next to a
  // 60 dB stronger signal eigenvalue; a Frobenius-relative test would stop far too early for them).
  const double tol2 = 1e-28;
  int& s_dirty = *reinterpret_cast<int*>(smem_raw + lds.dirty);   // lives in the dynamic LDS carve (keeps its base 16-B aligned)
  int sweep = 0;
  long long cyc_p = 0, cyc_u = 0;                  // phase instrumentation (ISAC_DEBUG): cycles of thread 0
  for (; sweep < max_sweeps; ++sweep) {
    if (tid == 0) s_dirty = 0;
    __syncthreads();
    for (int round = 0; round < n - 1; ++round) {
      const long long t_p0 = clock64();
      // ---- P: rotation parameters of the h disjoint pairs
      for (int kk = tid; kk < h; kk += nt) {
        int p, q;
        rr_pair(round, kk, n, p, q);
        rp[kk] = p; rq[kk] = q;
        const c64 beta = H[p + n * q];
        const double hpp = H[p + n * p].re, hqq = H[q + n * q].re;
        const double d = hqq - hpp;
        const double m2 = beta.re * beta.re + beta.im * beta.im;
        double c = 1.0;
        c64 g = mk(0.0, 0.0);
        if (m2 > tol2 * fabs(hqq * hpp)) s_dirty = 1;
        if (m2 > 0.0) {
          // u = sign(d) 2 / (|d| + sqrt(d^2 + 4 m2)),  c = 1 / sqrt(1 + u^2 m2): reciprocal square roots / reciprocals
          // from the hardware estimates + Newton steps (~350 cycles) instead of two sqrt and two divides (~520)
          const double x = ::fma(d, d, 4.0 * m2);
          double rs = __builtin_amdgcn_rsq(x);
          rs = ::fma(::fma(-0.5 * x * rs, rs, 0.5), rs, rs);
          rs = ::fma(::fma(-0.5 * x * rs, rs, 0.5), rs, rs);
          const double den = fabs(d) + x * rs;                    // |d| + sqrt(x) > 0
          double rden = __builtin_amdgcn_rcp(den);
          rden = rden * ::fma(-den, rden, 2.0);
          rden = rden * ::fma(-den, rden, 2.0);
          const double u = copysign(2.0, d) * rden;
          const double y = ::fma(u * u, m2, 1.0);
          double ry = __builtin_amdgcn_rsq(y);
          ry = ::fma(::fma(-0.5 * y * ry, ry, 0.5), ry, ry);
          ry = ::fma(::fma(-0.5 * y * ry, ry, 0.5), ry, ry);
          c = ry;
          const double cu = c * u;
          g = mk(cu * beta.re, cu * beta.im);
        }
        rc[kk] = c;
        rg[kk] = g;
      }
      __syncthreads();
      const long long t_u0 = clock64();
      cyc_p += t_u0 - t_p0;
      // ---- U: two-sided 2x2 block updates of H, column rotations of V
      // (updating only the blocks a <= b and storing only the upper triangle halves H's LDS traffic but leaves half of
      // the threads idle and adds index selects: measured 20 % slower)
      for (int blk = tid; blk < h * h; blk += nt) {
        const int a = blk % h, b = blk / h;
        const int pa = rp[a], qa = rq[a], pb = rp[b], qb = rq[b];
        const double ca = rc[a], cb = rc[b];
        const c64 ga = rg[a], gb = rg[b];
        const c64 h00 = H[pa + n * pb], h01 = H[pa + n * qb], h10 = H[qa + n * pb], h11 = H[qa + n * qb];
        // T = B J_b
        const c64 gbc = conj(gb);
        const c64 t00 = h00 * cb - h01 * gbc, t01 = h00 * gb + h01 * cb;
        const c64 t10 = h10 * cb - h11 * gbc, t11 = h10 * gb + h11 * cb;
        // B' = J_a^H T,  J_a^H = [[ca, -ga], [conj(ga), ca]]
        const c64 gac = conj(ga);
        c64 b00 = t00 * ca - ga * t10, b01 = t01 * ca - ga * t11;
        c64 b10 = gac * t00 + t10 * ca, b11 = gac * t01 + t11 * ca;
        if (a == b) { b01 = mk(0.0, 0.0); b10 = mk(0.0, 0.0); b00.im = 0.0; b11.im = 0.0; }
        H[pa + n * pb] = b00; H[pa + n * qb] = b01; H[qa + n * pb] = b10; H[qa + n * qb] = b11;
      }
      for (int it = tid; it < n * h; it += nt) {
        const int row = it % n, k = it / n;
        const int p = rp[k], q = rq[k];
        const double c = rc[k];
        const c64 g = rg[k];
        const c64 vp = V[row + n * p], vq = V[row + n * q];
        V[row + n * p] = vp * c - vq * conj(g);
        V[row + n * q] = vp * g + vq * c;
      }
      __syncthreads();
      cyc_u += clock64() - t_u0;
    }
    const int dirty = s_dirty;
    __syncthreads();                      // everyone has read the flag before thread 0 clears it again
    if (!dirty) { ++sweep; break; }
  }
  for (int i = tid; i < A; i += nt) w_out[i] = H[i + n * i].re / scl;     // (power of two: exact)
  for (int i = tid; i < A * A; i += nt) {
    int r = i % A, c = i / A;
    V_out[i] = V[r + n * c];
  }
  if (tid == 0 && info) { info->status = sweep; info->cyc_a = (int)(cyc_p >> 6); info->cyc_b = (int)(cyc_u >> 6); info->cyc_ql = 0; info->cyc_replay = 0; info->rotations = kEighRouteJacobi; }
}

// ---------------------------------------------------------------- Hermitian eigensolver II: Householder tridiagonalisation + implicit QL
// eig(Ra) of music.m:19 the LAPACK way (zhetd2 -> zungtr -> tql2), two launches on one stream, state in an L2-resident
// global scratch (working matrix in LDS while n <= 64):
//   K1  n-1 Householder reflectors reduce H to a REAL symmetric tridiagonal (d, e): eigh_tridiag_small_kernel (n <= 64),
//       eigh_tridiag_dist_kernel (n <= kTdMaxN) or eigh_tridiag_fused_kernel, see launch_tridiag
//   K2  eigh_formq_ql_kernel  independent workgroups side by side:
//         block 0: Q = H_0 ... H_{n-2} formed explicitly in Z (zungtr)
//         block 1: one wavefront runs the strictly sequential implicit-shift QL recurrence on (d, e) ALONE -- one
//                  dependent fp64 chain per plane rotation, no matrix traffic -- records every rotation (c, s) and
//                  publishes the sweeps one by one
//         blocks 2..: replay the published rotations on their rows of Z (rows are independent; held in LDS) as soon as
//                  zungtr has finished -- one CU streams a 1 MB Z once per sweep at ~29 B/clk, and that bandwidth, not
//                  the arithmetic, bounded the version in which one workgroup did everything
//       (eigh_replay_kernel: the same replay as a third launch when the rows do not fit LDS.)
// A = 256: 99 ms (Jacobi in global memory) -> 27 ms (one workgroup doing everything) -> 11 ms; A = 64: 0.86 ms (Jacobi 1.4).
// ---- n > 64, one pass over the trailing matrix per reflector instead of two.  zhetd2 reads A22 for p = tau A22 v and then reads AND writes it for
// A22 -= v w' + w v'; the matrix (1 MB at n = 256) streams from L2 through one CU, and that traffic is half of the kernel.  Here the rank-2
// update of step k - 1 is carried as a PENDING pair (v, w) and applied while the matrix-vector product of step k walks the matrix:
//   (a) column k gets the pending update by itself (O(n)) -> d[k], the new reflector v', tau';
//   (b) one pass over rows / columns > k:  a' = a - v_i conj(w_j) - w_i conj(v_j);  store a';  acc_i += a' v'_j   (one read + one write per element);
//   (c) w' = tau' acc + alpha v'  becomes the pending pair of step k + 1.
// Element for element the arithmetic is that of the two-pass form (same update expression, same partial-sum order of the product): d, e,
// tau and the reflectors come out bit-identical.
__global__ __launch_bounds__(1024) void eigh_tridiag_fused_kernel(const c64* __restrict__ Hin, int n, void* scratch, EighInfo* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  EighScratch S(scratch, n);
  const TridiagFusedLds lds = TridiagFusedLds::of(n);
  c64* M = S.M;                                     // [n x n] column-major working matrix (reflectors end up below the subdiagonal)
  c64* sv = reinterpret_cast<c64*>(smem_raw + lds.sv);         // pending reflector (zero before the first step)
  c64* sw = reinterpret_cast<c64*>(smem_raw + lds.sw);
  c64* sn = reinterpret_cast<c64*>(smem_raw + lds.sn);
  c64* spart = reinterpret_cast<c64*>(smem_raw + lds.spart);
  double* sred = reinterpret_cast<double*>(smem_raw + lds.sred);
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wid = tid >> 6, nw = nt >> 6;
  auto block_sum2 = [&](double a, double b, double& oa, double& ob) {   // sum over the workgroup of two values
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_down(a, o); b += __shfl_down(b, o); }
    __syncthreads();
    if (lane == 0) { sred[wid] = a; sred[16 + wid] = b; }
    __syncthreads();
    double ta = 0.0, tb = 0.0;
    for (int w = 0; w < nw; ++w) { ta += sred[w]; tb += sred[16 + w]; }
    oa = ta; ob = tb;
  };
  const long long t_start = clock64();
  const double scl = eigh_safe_scale(Hin, n * n, sred);
  for (int i = tid; i < n * n; i += nt) M[i] = Hin[i] * scl;
  for (int i = tid; i < n; i += nt) sv[i] = sw[i] = mk(0.0, 0.0);
  if (tid == 0) *S.scale = scl;
  if (tid < 8) S.cnt[tid] = 0;                      // publication counters of the next two stages
  __syncthreads();
  constexpr int rw_shift = 8, RW = 1 << rw_shift;   // row tile of the pass
  for (int k = 0; k < n - 1; ++k) {                 // zhetd2, lower
    const int m = n - k - 1;                        // trailing size, rows/cols k+1 .. n-1
    // (a) column k, rows k .. n-1: the pending update
    {
      const c64 wk = sw[k], vk = sv[k];
      for (int i = k + tid; i < n; i += nt) M[i + n * k] = M[i + n * k] - mul_conj(sv[i], wk) - mul_conj(sw[i], vk);
    }
    __syncthreads();
    double xn2 = 0.0, dummy = 0.0;
    for (int i = k + 2 + tid; i < n; i += nt) { const c64 x = M[i + n * k]; xn2 += x.re * x.re + x.im * x.im; }
    double xnorm2, unused;
    block_sum2(xn2, dummy, xnorm2, unused);
    const c64 alpha = M[k + 1 + n * k];
    const auto [beta, tau, scale] = zlarfg<false>(alpha, xnorm2);
    for (int i = k + 1 + tid; i < n; i += nt) {
      const c64 vi = (i == k + 1) ? mk(1.0, 0.0) : M[i + n * k] * scale;
      sn[i] = vi;
      if (i > k + 1) M[i + n * k] = vi;             // keep the reflector for zungtr
    }
    if (tid == 0) { S.d[k] = M[k + n * k].re; S.e[k] = beta; S.tau[k] = tau; }
    __syncthreads();
    // (b) rows / columns k+1 .. n-1: pending update applied, product with the new reflector accumulated (thread = row i, column quarter jq:
    // rows are coalesced across lanes, the four quarters of a row are summed through LDS -- the mapping and summation order of the unfused kernel)
    {
      const int rows_pt = (m + RW - 1) >> rw_shift;
      const int G = nt >> rw_shift;
      const int jq = tid >> rw_shift, il = tid & (RW - 1);
      const int jlen = (m + G - 1) / G;
      const int j0 = k + 1 + jq * jlen, j1 = min(n, j0 + jlen);
      for (int rr = 0; rr < rows_pt; ++rr) {
        const int i = k + 1 + il + RW * rr;
        c64 a0 = mk(0.0, 0.0), a1 = a0, a2 = a0, a3 = a0;
        if (i < n) {
          const c64 vi = sv[i], wi = sw[i];
          c64* Mi = M + i;
          int j = j0;
          for (; j + 4 <= j1; j += 4) {
            c64 e[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) e[u] = Mi[(long long)n * (j + u)];
#pragma unroll
            for (int u = 0; u < 4; ++u) { e[u] = e[u] - mul_conj(vi, sw[j + u]) - mul_conj(wi, sv[j + u]); Mi[(long long)n * (j + u)] = e[u]; }
            a0 = fma(e[0], sn[j], a0); a1 = fma(e[1], sn[j + 1], a1); a2 = fma(e[2], sn[j + 2], a2); a3 = fma(e[3], sn[j + 3], a3);
          }
          for (; j < j1; ++j) {
            const c64 e = Mi[(long long)n * j] - mul_conj(vi, sw[j]) - mul_conj(wi, sv[j]);
            Mi[(long long)n * j] = e;
            a0 = fma(e, sn[j], a0);
          }
          spart[jq * n + i] = (a0 + a1) + (a2 + a3);
        }
      }
      __syncthreads();                                      // every read of the pending pair is done: sv / sw can take the new one
      if (tau.re != 0.0 || tau.im != 0.0) {
        for (int i = k + 1 + tid; i < n; i += nt) {
          c64 acc = spart[i];
          for (int gq = 1; gq < G; ++gq) acc = acc + spart[gq * n + i];
          sw[i] = tau * acc;                                // p
        }
      }
    }
    __syncthreads();
    if (tau.re != 0.0 || tau.im != 0.0) {
      // alpha2 = -1/2 tau (p^H v);  w = p + alpha2 v
      double pr = 0.0, pi = 0.0;
      for (int i = k + 1 + tid; i < n; i += nt) { const c64 t = mul_conj(sn[i], sw[i]); pr += t.re; pi += t.im; }
      double sr, si;
      block_sum2(pr, pi, sr, si);
      const c64 a2 = mk(-0.5, 0.0) * (tau * mk(sr, si));
      __syncthreads();
      for (int i = k + 1 + tid; i < n; i += nt) { const c64 vi = sn[i]; sw[i] = sw[i] + a2 * vi; sv[i] = vi; }
    } else {
      for (int i = k + 1 + tid; i < n; i += nt) sv[i] = sw[i] = mk(0.0, 0.0);   // H_k = I: nothing pending
    }
    __syncthreads();
  }
  if (tid == 0) {
    const c64 c = M[n - 1 + n * (n - 1)] - mul_conj(sv[n - 1], sw[n - 1]) - mul_conj(sw[n - 1], sv[n - 1]);   // the last pending update
    S.d[n - 1] = c.re; S.e[n - 1] = 0.0;
    if (info) { info->cyc_a = (int)((clock64() - t_start) >> 6); info->sticky = 0; }
  }
}

// ---- 64 < n <= 256: the reduction DISTRIBUTED over ceil(n / 4) single-wavefront workgroups that hold the whole working matrix in registers.
// The one-workgroup kernels above stream the trailing matrix (1 MB at n = 256) from L2 through ONE compute unit once per reflector: 3.1-3.2 ms at
// n = 256, all of it that traffic.  Here wavefront q owns the 4 columns 4 q .. 4 q + 3 -- ALL their rows, both triangles: lane (c, rg) keeps the rows
// i = rg, rg + 16, ... of column 4 q + c in 16 complex registers -- so that, the matrix being Hermitian, p_j = tau sum_i conj(a_ij) v_i needs nothing but
// the owner's registers and the reflector, and the rank-2 update a_ij -= v_i conj(w_j) + w_i conj(v_j) nothing but v and w.  What crosses wavefronts per
// reflector is ONE exchange: every wavefront publishes its 4 entries of p and -- the owner -- the next column as it stands; from those, every
// wavefront forms w, the updated next column, its norm, zlarfg and the next reflector REDUNDANTLY (lane l: rows l, l + 64, l + 128, l + 192; identical
// instructions on identical data: identical bits), so the chain per reflector is  registers -> publish -> poll -> O(n) vector work -> registers  with no
// workgroup barrier and no pass over a matrix in memory.
//   Exchange protocol (placement-independent; MI355X guide, inter-workgroup visibility, form R2): the data carry their own tags.  Every double
// travels as one 16-byte write-through (sc1) store of two 8-byte granules {low word, tag}, {high word, tag}, tag = launch epoch << 12 | step -- no flag,
// no fence, no reset between launches; the consumer re-reads the 64 bytes of each of its rows (p_i and the next column's entry) with sc1 loads until
// all tags match.  Two parities of the area alternate: a wavefront can overwrite parity k & 1 at step k + 2 only after it has consumed every other
// wavefront's step k + 1, which they publish after reading step k.  A wavefront returns after the step that consumed its last column; a poll that
// sees no progress for ~2 s gives up with kEighTridiagTimeout.
//   History (n = 256, profiles/r04_tridiag_dist.txt): 16 workgroups of 256 threads, agent-scope atomics + one step stamp per workgroup behind
// s_waitcnt 1.0 ms (with __threadfence() instead 2.8 ms); tagged granules 0.9 ms -- 58 % of it the O(n) vector work, a chain of ~550 dependent
// instructions through two workgroup-wide sums per reflector; this form: the sums stay inside the wavefront (DPP), four independent rows per lane.
constexpr int kTdMaxN = 256;
constexpr unsigned kTdRowBytes = 64, kTdParBytes = kTdMaxN * kTdRowBytes, kTdMxBytes = 2048;      // per row: p_i (32 B) | column entry (32 B)
static_assert(EighScratch::kXchBytes == kTdMxBytes + 2 * kTdParBytes, "exchange area");
__device__ __forceinline__ void td_put(__amdgpu_buffer_rsrc_t rs, unsigned off, double v, unsigned tag, bool near = false) {
  const u32x4_t q = {(unsigned)__double2loint(v), tag, (unsigned)__double2hiint(v), tag};
  if (near) __builtin_amdgcn_raw_buffer_store_b128(q, rs, (int)off, 0, 0);             // stays in this XCD's L2: readers on the same XCD only
  else __builtin_amdgcn_raw_buffer_store_b128(q, rs, (int)off, 0, /*sc1*/ 16);          // write-through: visible at any placement
}
__device__ __forceinline__ bool td_get(__amdgpu_buffer_rsrc_t rs, unsigned off, unsigned tag, double& v) {
  const u32x4_t q = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)off, 0, /*sc1*/ 16);
  v = __hiloint2double((int)q.z, (int)q.x);
  return q.y == tag && q.w == tag;
}
__device__ __forceinline__ double row16_sum_dpp(double x) {      // every lane: the sum over its row of 16 lanes
  x += dpp_move<0xB1, 0xf>(x);
  x += dpp_move<0x4E, 0xf>(x);
  x += dpp_move<0x124, 0xf>(x);
  x += dpp_move<0x128, 0xf>(x);
  return x;
}
__global__ __launch_bounds__(256) void eigh_tridiag_dist_kernel(const c64* __restrict__ Hin, int n, void* scratch, EighInfo* __restrict__ info, unsigned base,
                                                                      int stride, int slot, int far_only, int force_abort) {
  if ((int)(blockIdx.x % (unsigned)stride) != slot) return;
  if (force_abort) { if (threadIdx.x == 0 && info) eigh_mark_tridiag_timeout(info); return; }   // test hook (ISAC_EIG_FORCE_TRIDIAG_TIMEOUT): behave like an exchange that timed out
  __shared__ __attribute__((aligned(16))) c64 sv[2][kTdMaxN];      // the reflector of the step, by parity   (sv, sw: every wavefront writes the same bits)
  __shared__ __attribute__((aligned(16))) c64 sw[kTdMaxN];         // w of the step
  __shared__ __attribute__((aligned(16))) c64 scol4[4][kTdMaxN];   // per wavefront: the owner's next column, row by row
  __shared__ __attribute__((aligned(16))) c64 sp[2][kTdMaxN];      // the exchange as polled (wavefront w: rows 64 w ..), by parity: p ...
  __shared__ __attribute__((aligned(16))) c64 sc[2][kTdMaxN];      // ... and the next column
  __shared__ int s_abort;
  const int wid = threadIdx.x >> 6;
  const int g = (int)(blockIdx.x / (unsigned)stride), G = (n + 15) >> 4, q = 4 * g + wid, Q = (n + 3) >> 2;
  const int lane = threadIdx.x & 63;
  c64* scol = scol4[wid];
  if (threadIdx.x == 0) s_abort = 0;
  const int c = lane >> 4, rg = lane & 15, j = 4 * q + c;
  EighScratch S(scratch, n);
  const __amdgpu_buffer_rsrc_t xr = buffer_of(S.xch, (unsigned)EighScratch::kXchBytes);
  const bool writer = g == G - 1 && wid == 0;                        // (alive to the last step) stores d, e, tau and the reflectors
  const long long t_start = clock64();
  auto give_up = [&](const long long t0, int& spins) -> bool {       // (wave-uniform) ~2 s without progress
    if ((++spins & 255) != 0 || (long long)wall_clock64() - t0 < 200000000ll) return false;
    if (lane == 0) s_abort = 1;
    return true;
  };
  // ---- load: my columns' rows; the safe scale needs the maximum over the whole matrix: first exchange
  c64 a[16];
  double mx = 0.0;
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int i = 16 * u + rg;
    a[u] = (i < n && j < n) ? Hin[i + (long long)n * j] : mk(0.0, 0.0);
    mx = fmax(mx, fmax(fabs(a[u].re), fabs(a[u].im)));
  }
  double scl = 1.0;
  bool near = false;                                                 // every wavefront of the launch runs on ONE XCD (seen in the first exchange): the exchange may stay in its L2
  c64 col[4];                                                        // column 0 (lane l: rows l + 64 r): every wavefront derives the first reflector itself
#pragma unroll
  for (int r = 0; r < 4; ++r) col[r] = lane + 64 * r < n ? Hin[lane + 64 * r] : mk(0.0, 0.0);
  {
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
    unsigned xcc = 0;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    xcc &= 15;
    if (lane == 0) { td_put(xr, 32u * (unsigned)q, mx, base + 1); td_put(xr, 32u * (unsigned)q + 16, (double)xcc, base + 1); }
    double t = 0.0;
    const long long t0 = (long long)wall_clock64();
    int spins = 0;
    for (;;) {
      asm volatile("" ::: "memory");
      double m = 0.0, x = (double)xcc;
      const bool ok = lane >= Q || (td_get(xr, 32u * (unsigned)lane, base + 1, m) && td_get(xr, 32u * (unsigned)lane + 16, base + 1, x));
      if (__all(ok)) { t = lane < Q ? m : 0.0; near = !far_only && __all(x == (double)xcc); break; }
      if (give_up(t0, spins)) break;
    }
    for (int o = 32; o > 0; o >>= 1) t = fmax(t, __shfl_xor(t, o));
    __syncthreads();
    if (s_abort) { if (threadIdx.x == 0 && info) eigh_mark_tridiag_timeout(info); return; }
    scl = eigh_scale_of(t);
#pragma unroll
    for (int u = 0; u < 16; ++u) a[u] = a[u] * scl;
#pragma unroll
    for (int r = 0; r < 4; ++r) col[r] = col[r] * scl;
    if (writer) {
      if (lane == 0) *S.scale = scl;
      if (lane < 8) S.cnt[lane] = 0;                                 // publication counters of the next two stages
    }
  }
  // the reflector of step k2 from its column: into vn (registers) and sv[k2 & 1] (LDS), tau returned; d, e, tau and the reflector stored by the writer
  c64 vcur[4];
  auto derive = [&](int k2, const c64 (&ci)[4], const c64 alpha /* row k2 + 1 */, const double dd /* row k2, real part */) -> c64 {
    double xn2 = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) { const int i = lane + 64 * r; if (i > k2 + 1 && i < n) xn2 += ci[r].re * ci[r].re + ci[r].im * ci[r].im; }
    xn2 = wave_sum_dpp(xn2);
    const auto [beta, tau, scale] = zlarfg<true>(alpha, xn2);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = lane + 64 * r;
      const bool below = i > k2 + 1 && i < n;
      const c64 vi = i == k2 + 1 ? mk(1.0, 0.0) : (below ? ci[r] * scale : mk(0.0, 0.0));
      vcur[r] = vi;
      sv[k2 & 1][i] = vi;
      if (writer && below) S.M[i + (long long)n * k2] = vi;          // the reflector, where zungtr / the back-transform expect it
    }
    if (writer && lane == 0) { S.d[k2] = dd; S.e[k2] = beta; S.tau[k2] = tau; }
    return tau;
  };
  c64 tau = derive(0, col, Hin[1] * scl, Hin[0].re * scl);
  long long c_pub = 0, c_poll = 0, c_vec = 0, c_upd = 0;          // phase instrumentation (ISAC_DEBUG): cycles of the last wavefront
  for (int k = 0; k < n - 1; ++k) {
    const long long c0 = clock64();
    const int par = k & 1;
    const c64* v = sv[par];
    const unsigned tag = base + 2 + (unsigned)k;
    const unsigned area = kTdMxBytes + (unsigned)par * kTdParBytes;
    // ---- the owner of column k + 1 publishes it as it stands (the update of step k - 1 is in), spread over the wavefront through LDS
    if (q == ((k + 1) >> 2)) {                                       // (wave-uniform)
      if (c == ((k + 1) & 3)) {
#pragma unroll
        for (int u = 0; u < 16; ++u) scol[16 * u + rg] = a[u];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = lane + 64 * r;
        if (i > k && i < n) {
          const c64 x = scol[i];
          td_put(xr, area + kTdRowBytes * (unsigned)i + 32, x.re, tag, near);
          td_put(xr, area + kTdRowBytes * (unsigned)i + 48, x.im, tag, near);
        }
      }
    }
    // ---- p_j = tau sum_i conj(a_ij) v_i over my columns
    {
      c64 acc0 = mk(0.0, 0.0), acc1 = acc0;
#pragma unroll
      for (int u = 0; u < 16; u += 2) {
        acc0 = fma(conj(a[u]), v[16 * u + rg], acc0);
        acc1 = fma(conj(a[u + 1]), v[16 * (u + 1) + rg], acc1);
      }
      const c64 pj = tau * mk(row16_sum_dpp(acc0.re + acc1.re), row16_sum_dpp(acc0.im + acc1.im));
      if (rg < 2 && j > k && j < n) td_put(xr, area + kTdRowBytes * (unsigned)j + 16 * (unsigned)rg, rg == 0 ? pj.re : pj.im, tag, near);
    }
    if (g != G - 1 && 16 * g + 15 == k + 1) return;                  // that was my workgroup's last column
    // ---- the exchange: wavefront w polls the rows 64 w .. 64 w + 63 for the workgroup
    const long long c1 = clock64();
    c_pub += c1 - c0;
    {
      const int i = 64 * wid + lane;
      const bool alive = i > k && i < n;
      c64 pr = mk(0.0, 0.0), cr = pr;
      if (__any(alive)) {                                            // (wave-uniform)
        const long long t0 = (long long)wall_clock64();
        int spins = 0;
        const unsigned off = area + kTdRowBytes * (unsigned)i;
        for (;;) {
          asm volatile("" ::: "memory");
          bool ok = true;
          if (alive) {
            const bool o0 = td_get(xr, off, tag, pr.re), o1 = td_get(xr, off + 16, tag, pr.im);
            const bool o2 = td_get(xr, off + 32, tag, cr.re), o3 = td_get(xr, off + 48, tag, cr.im);
            ok = o0 && o1 && o2 && o3;
          }
          if (__all(ok)) break;
          if (give_up(t0, spins)) break;
        }
      }
      sp[par][i] = pr;
      sc[par][i] = cr;
    }
    __syncthreads();
    if (s_abort) { if (threadIdx.x == 0 && info) eigh_mark_tridiag_timeout(info); return; }
    c64 pi[4], ci[4];
    bool live[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { pi[r] = sp[par][lane + 64 * r]; ci[r] = sc[par][lane + 64 * r]; live[r] = lane + 64 * r > k && lane + 64 * r < n; }
    const long long c2 = clock64();
    c_poll += c2 - c1;
    double sr = 0.0, si = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) { const c64 t = mul_conj(vcur[r], pi[r]); sr += t.re; si += t.im; }   // conj(p_i) v_i  (dead rows: p_i = 0)
    sr = wave_sum_dpp(sr); si = wave_sum_dpp(si);
    const c64 a2 = mk(-0.5, 0.0) * (tau * mk(sr, si));               // -1/2 tau (p^H v)
    const c64 wk1 = sp[par][k + 1] + a2;                             // (v_{k+1} = 1)
    c64 cn[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const c64 wi = live[r] ? pi[r] + a2 * vcur[r] : mk(0.0, 0.0);
      sw[lane + 64 * r] = wi;
      cn[r] = ci[r] - mul_conj(vcur[r], wk1) - wi;                   // column k+1 after the update (row k+1: its diagonal)
    }
    const double d_next = sc[par][k + 1].re - 2.0 * wk1.re;          // row k+1 of the updated column (v = 1, w = wk1): the next diagonal entry
    if (k + 1 == n - 1) {
      if (writer && lane == 0) { S.d[n - 1] = d_next; S.e[n - 1] = 0.0; }
      break;
    }
    const c64 v2 = v[k + 2];                                         // row k+2 of it, formed by every lane (broadcast reads): the next alpha
    const c64 alpha_next = sc[par][k + 2] - mul_conj(v2, wk1) - (sp[par][k + 2] + a2 * v2);
    const c64 tau_next = derive(k + 1, cn, alpha_next, d_next);      // (overwrites vcur; the update below reads v_k from LDS)
    const long long c3 = clock64();
    c_vec += c3 - c2;
    // ---- rank-2 update of my columns
    if (j > k && j < n) {
      const c64 wj = sw[j], vj = v[j];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int i = 16 * u + rg;
        a[u] = a[u] - mul_conj(v[i], wj) - mul_conj(sw[i], vj);
      }
    }
    tau = tau_next;
    c_upd += clock64() - c3;
  }
  if (writer && lane == 0 && info) {
    info->cyc_a = (int)((clock64() - t_start) >> 6);
    info->tri_a = (int)(c_pub >> 6); info->tri_b = (int)(c_poll >> 6); info->tri_c = (int)(c_vec >> 6); info->tri_d = (int)(c_upd >> 6);
  }
}

// ---- n <= 64: the same zhetd2 reduction on four wavefronts with TWO barriers per step instead of ten.  Lane i owns row i; every wave
// derives the reflector of the step redundantly (column read, norm by a wave reduction, zlarfg scalars) and keeps its own copy of v and
// w in LDS for broadcast reads, so nothing of that needs a workgroup barrier; wave g handles the columns j = k+1+g, k+5+g, ... of the
// matrix-vector product (partials exchanged through LDS: barrier 1) and of the rank-2 update (barrier 2 before the next step reads the
// updated column).  The matrix lives in LDS, the reflectors go straight to the scratch zungtr reads.  222 -> ~120 us at n = 64
// (host-call time of the whole eigensolver 0.905 -> 0.807 ms).
// (Round 4 tried the matrix in REGISTERS: wave w owns the columns j = w (mod 4), the 63 steps unrolled, per-column operands by v_readlane, LDS only for
// the new reflector and the partial products -- 35 000 instructions, 128.9 us against this kernel's 129.3: the step is bound by what ONE wave can issue
// (~8 cycles per instruction: ~550 instructions per step either way) and by the serial zlarfg chain (sqrt + three fp64 divides + three DPP sums),
// not by the LDS traffic it removed.  profiles/r04_negative_results.txt.)
__global__ __launch_bounds__(64 * kTriWaves) void eigh_tridiag_small_kernel(const c64* __restrict__ Hin, int n, void* scratch, EighInfo* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  constexpr int NW = kTriWaves;
  EighScratch S(scratch, n);
  const TridiagSmallLds lds = TridiagSmallLds::of(n);
  c64* M = reinterpret_cast<c64*>(smem_raw + lds.M);
  c64* spart = reinterpret_cast<c64*>(smem_raw + lds.spart);
  c64* svw = reinterpret_cast<c64*>(smem_raw + lds.svw);
  double* sred = reinterpret_cast<double*>(smem_raw + lds.sred);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  c64* my_v = svw + (size_t)wid * 128;
  c64* my_w = my_v + 64;
  const long long t_start = clock64();
  const double scl = eigh_safe_scale(Hin, n * n, sred);
  for (int i = tid; i < n * n; i += 64 * NW) M[i] = Hin[i] * scl;
  if (tid == 0) *S.scale = scl;
  if (tid < 8) S.cnt[tid] = 0;                                    // publication counters of the next two stages
  __syncthreads();
  auto wave_sum = [](double x) { return wave_sum_dpp(x); };
  long long c_refl = 0, c_mv = 0, c_upd = 0;                      // phase instrumentation (ISAC_DEBUG): cycles of thread 0
  for (int k = 0; k < n - 1; ++k) {                               // zhetd2, lower
    const long long c0 = clock64();
    const bool below = lane > k + 1 && lane < n;
    const c64 xi = below ? M[lane + n * k] : mk(0.0, 0.0);
    const c64 alpha = M[k + 1 + n * k];                           // (broadcast read)
    const double xnorm2 = wave_sum(xi.re * xi.re + xi.im * xi.im);
    const auto [beta, tau, scale] = zlarfg<false>(alpha, xnorm2);
    const c64 vi = lane == k + 1 ? mk(1.0, 0.0) : (below ? xi * scale : mk(0.0, 0.0));
    my_v[lane] = vi;                                              // (wave-private: no barrier, LDS operations of a wave are in order)
    if (wid == 0) {
      if (below) S.M[lane + n * k] = vi;                          // the reflector, where zungtr expects it
      if (lane == 0) { S.d[k] = M[k + n * k].re; S.e[k] = beta; S.tau[k] = tau; }
    }
    const long long c1 = clock64();
    c_refl += c1 - c0;
    if (tau.re != 0.0 || tau.im != 0.0) {                         // (uniform)
      // p = tau A22 v: my columns' share of row `lane`
      // (four columns per trip, their LDS reads issued together: a single dependent chain waits ~130 cycles per column)
      c64 acc = mk(0.0, 0.0);
      if (lane < n) {
        c64 a0 = mk(0.0, 0.0), a1 = a0, a2_ = a0, a3 = a0;
        int j = k + 1 + wid;
        for (; j + 3 * NW < n; j += 4 * NW) {
          const c64 m0 = M[lane + n * j], m1 = M[lane + n * (j + NW)], m2 = M[lane + n * (j + 2 * NW)], m3 = M[lane + n * (j + 3 * NW)];
          const c64 v0 = my_v[j], v1 = my_v[j + NW], v2 = my_v[j + 2 * NW], v3 = my_v[j + 3 * NW];
          a0 = fma(m0, v0, a0); a1 = fma(m1, v1, a1); a2_ = fma(m2, v2, a2_); a3 = fma(m3, v3, a3);
        }
        for (; j < n; j += NW) a0 = fma(M[lane + n * j], my_v[j], a0);
        acc = (a0 + a1) + (a2_ + a3);
      }
      spart[wid * 64 + lane] = acc;
      __syncthreads();
      c_mv += clock64() - c1;
      c64 psum = mk(0.0, 0.0);
#pragma unroll
      for (int g = 0; g < NW; ++g) psum = psum + spart[g * 64 + lane];                    // fixed order: every wave forms the same p
      const c64 pi = lane > k && lane < n ? tau * psum : mk(0.0, 0.0);
      const c64 t = mul_conj(vi, pi);                             // conj(p_i) v_i
      const c64 a2 = mk(-0.5, 0.0) * (tau * mk(wave_sum(t.re), wave_sum(t.im)));   // -1/2 tau (p^H v)   (zhetd2: zdotc(tau-scaled p, v))
      const c64 wi = pi + a2 * vi;
      my_w[lane] = wi;
      // A22 -= v w^H + w v^H on my columns
      if (lane > k && lane < n) {
        int j = k + 1 + wid;
        for (; j + 3 * NW < n; j += 4 * NW) {
          c64 m[4], wj[4], vj[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) { m[u] = M[lane + n * (j + NW * u)]; wj[u] = my_w[j + NW * u]; vj[u] = my_v[j + NW * u]; }
#pragma unroll
          for (int u = 0; u < 4; ++u) M[lane + n * (j + NW * u)] = m[u] - mul_conj(vi, wj[u]) - mul_conj(wi, vj[u]);
        }
        for (; j + NW < n; j += 2 * NW) {                          // (two columns per trip for the short tails)
          const c64 m0 = M[lane + n * j], m1 = M[lane + n * (j + NW)];
          const c64 w0 = my_w[j], w1 = my_w[j + NW], v0 = my_v[j], v1 = my_v[j + NW];
          M[lane + n * j] = m0 - mul_conj(vi, w0) - mul_conj(wi, v0);
          M[lane + n * (j + NW)] = m1 - mul_conj(vi, w1) - mul_conj(wi, v1);
        }
        for (; j < n; j += NW) M[lane + n * j] = M[lane + n * j] - mul_conj(vi, my_w[j]) - mul_conj(wi, my_v[j]);
      }
    }
    __syncthreads();
    c_upd += clock64() - c1;
  }
  if (tid == 0) {
    S.d[n - 1] = M[n - 1 + n * (n - 1)].re; S.e[n - 1] = 0.0;
    if (info) { info->cyc_a = (int)((clock64() - t_start) >> 6); info->sticky = 0; info->tri_a = (int)(c_refl >> 6); info->tri_b = (int)(c_mv >> 6); info->tri_c = (int)(c_upd >> 6); }
  }
}

template <bool LDS, bool LIVE>
__device__ __forceinline__ void eigh_replay_body(int n, const EighScratch& S, c64* __restrict__ V_out, char* smem_raw, int block,
                                                 int bt, EighInfo* __restrict__ info);

// block 0: zungtr; block 1 (first wavefront): tql2 recurrence, rotations recorded; blocks >= 2: live replay
__global__ __launch_bounds__(1024) void eigh_formq_ql_kernel(int n, void* scratch, double* __restrict__ w_out, EighInfo* __restrict__ info,
                                                             c64* __restrict__ V_out, int replay_bt, const int* __restrict__ ctl) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  if (ctl && ctl[0] == 1) return;                   // (grid-uniform) music_subspace_kernel has delivered the signal vectors: no full basis needed
  EighScratch S(scratch, n);
  const FormqQlLds lds = FormqQlLds::of(n);
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wid = tid >> 6, nw = nt >> 6;
  const long long t0 = clock64();
  if (blockIdx.x == 0) {
    // ---- Q (zungtr): Z = H_0 H_1 ... H_{n-2}, accumulated backwards
    const c64* M = S.M;
    c64* Z = S.Z;
    c64* sv = reinterpret_cast<c64*>(smem_raw + lds.sv);
    c64* sp = reinterpret_cast<c64*>(smem_raw + lds.sp);
    for (int i = tid; i < n * n; i += nt) Z[i] = mk((i % n) == (i / n) ? 1.0 : 0.0, 0.0);
    __syncthreads();
    for (int k = n - 2; k >= 0; --k) {
      const c64 tau = S.tau[k];
      if (tau.re == 0.0 && tau.im == 0.0) continue; // (uniform)
      for (int i = k + 1 + tid; i < n; i += nt) sv[i] = (i == k + 1) ? mk(1.0, 0.0) : M[i + n * k];
      __syncthreads();
      // u[j] = v^H Z[k+1:, j]: one wave per column (lanes along the column: coalesced), shuffle reduction
      for (int j = k + 1 + wid; j < n; j += nw) {
        c64 acc = mk(0.0, 0.0);
        for (int i = k + 1 + lane; i < n; i += 64) acc = fma(conj(sv[i]), Z[i + n * j], acc);
        for (int o = 32; o > 0; o >>= 1) { acc.re += __shfl_down(acc.re, o); acc.im += __shfl_down(acc.im, o); }
        if (lane == 0) sp[j] = tau * acc;
      }
      __syncthreads();
      for (int i = k + 1 + (tid & 255); i < n; i += 256) {
        const c64 vi = sv[i];
        for (int j = k + 1 + (tid >> 8); j < n; j += (nt >> 8)) Z[i + n * j] = Z[i + n * j] - vi * sp[j];
      }
      __syncthreads();
    }
    __threadfence();                                // Z complete and visible before the flag
    __syncthreads();
    if (tid == 0) {
      __hip_atomic_store(&S.cnt[3], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      if (info) info->cyc_b = (int)((clock64() - t0) >> 6);
    }
    return;
  }
  if (blockIdx.x >= 2) {                            // live replay blocks (only launched when the rows fit LDS)
    eigh_replay_body<true, true>(n, S, V_out, smem_raw, (int)blockIdx.x - 2, replay_bt, info);
    return;
  }
  if (wid != 0) return;
  // ---- implicit QL (tql2) on (d, e) only.  All 64 lanes compute the same scalars (no divergence, no broadcasts);
  // lanes only split the work in the split search, the backup copy and the flush of the recorded rotations.
  // A lone wavefront issues one instruction every ~5-8 cycles whatever the dependences (tools/latbench.hip: the whole
  // recurrence from registers = 160 cycles per rotation), so the loop is written for instruction count: (d, e) are
  // interleaved in one LDS array (one 16-byte read and one 16-byte write per rotation), no per-rotation underflow test
  // (a zero r^2 turns the carried values into NaNs, tested once after the sweep).
  c64* de = reinterpret_cast<c64*>(smem_raw + lds.de);     // (.re = d, .im = e)
  c64* bde = reinterpret_cast<c64*>(smem_raw + lds.bde);   // backup of the sweep window (r == 0 recovery)
  c64* rec = reinterpret_cast<c64*>(smem_raw + lds.rec);
  for (int i = lane; i < n; i += 64) de[i] = mk(S.d[i], S.e[i]);
  int sweeps = 0;
  long long nrot = 0;
  int overflow = 0;
  for (int l = 0; l < n && !overflow; ++l) {
    int iter = 0;
    while (true) {
      // first mm >= l with a negligible e[mm] (or n-1): 64 candidates per ballot instead of a serial scan
      // (a VALU -> SALU hand-off costs ~110 cycles on this chip, tools/latbench.hip)
      int mm = n - 1;
      for (int base = l; base < n - 1; base += 64) {
        const int j = base + lane;
        bool small = false;
        if (j < n - 1) small = fabs(de[j].im) <= 2.220446049250313e-16 * (fabs(de[j].re) + fabs(de[j + 1].re));
        const unsigned long long mask = __ballot(small);
        if (mask) { mm = base + __builtin_ctzll(mask); break; }
      }
      if (mm == l) break;
      if (++iter > 60) break;                       // (never reached for Hermitian input; keeps the loop bounded)
      if (sweeps >= S.desc_cap || nrot + (mm - l) + 8 > S.rot_cap) { overflow = 1; break; }
      for (int i = l + lane; i <= mm; i += 64) bde[i] = de[i];
      const c64 de_l = de[l];
      double g0 = (de[l + 1].re - de_l.re) / (2.0 * de_l.im);
      const double r0 = sqrt(g0 * g0 + 1.0);
      g0 = de[mm].re - de_l.re + de_l.im / (g0 + copysign(r0, g0));
      // ---- fast chase
      double g = g0, sn = 1.0, cs = 1.0, p = 0.0;
      {
        // one rotation; (dx, ex) = (d_i, e_i), dh = d_{i+1} before the rotation
        auto rotate = [&](int i, double dx, double ex, double dh) {
          const double f = sn * ex;
          const double b2 = (cs + cs) * ex;            // 2 b
          const double rr2 = ::fma(f, f, g * g);
          // 1/sqrt(rr2) from the hardware estimate y0 (~2^-23 relative) by one third-order step
          //   y = y0 (1 + h/2 + 3 h^2/8),  h = 1 - rr2 y0^2   (error ~ h^3 = 2^-69), instead of sqrt + two divides
          const double y0 = __builtin_amdgcn_rsq(rr2);
          const double h = ::fma(-rr2 * y0, y0, 1.0);
          const double inv = ::fma(y0 * h, ::fma(h, 0.375, 0.5), y0);
          sn = f * inv;
          cs = g * inv;
          const double g1 = dh - p;
          const double rr1 = ::fma(dx - g1, sn, cs * b2);
          p = sn * rr1;
          de[i + 1] = mk(g1 + p, rr2 * inv);           // d[i+1], e[i+1] = r
          g = ::fma(cs, rr1, -0.5 * b2);
          rec[mm - 1 - i] = mk(cs, sn);
        };
        // two rotations per trip (no register shuffling between them); operands are fetched one trip ahead
        int i = mm - 1;
        double d_hi = de[mm].re;
        c64 x0 = de[i], x1 = de[i > l ? i - 1 : l];
        for (; i - 1 >= l; i -= 2) {
          const c64 n0 = de[i - 2 >= l ? i - 2 : l], n1 = de[i - 3 >= l ? i - 3 : l];
          rotate(i, x0.re, x0.im, d_hi);
          rotate(i - 1, x1.re, x1.im, x0.re);
          d_hi = x1.re;
          x0 = n0; x1 = n1;
        }
        if (i >= l) rotate(i, x0.re, x0.im, d_hi);     // odd tail
      }
      bool underflow = false;
      if (__builtin_amdgcn_readfirstlane((int)!(g == g && p == p))) {
        // ---- tql2's r == 0 exit happened somewhere in this sweep (or the input holds a NaN): restore and redo it
        // carefully.  The recovery is carried as a 0/1 double (`lv`): once r == 0, the remaining rotations become
        // identities and every store writes back the value it found -- no branch on a VALU result inside the chain.
        for (int i = l + lane; i <= mm; i += 64) de[i] = bde[i];
        g = g0; sn = 1.0; cs = 1.0; p = 0.0;
        int i = mm - 1;
        double d_hi = de[mm].re, e_hi = de[mm].im;
        double e_i = de[i].im, d_i = de[i].re;
        double lv = 1.0, uf = 0.0;
        for (; i >= l; --i) {
          const int ip = i > l ? i - 1 : l;
          const double e_nx = de[ip].im, d_nx = de[ip].re;
          const double f = sn * e_i;
          const double b = cs * e_i;
          const double rr2 = ::fma(f, f, g * g);
          const double rs = (rr2 == 0.0) ? 1.0 : rr2;
          double inv = __builtin_amdgcn_rsq(rs);
          const double hrs = 0.5 * rs;
          inv = ::fma(::fma(-hrs * inv, inv, 0.5), inv, inv);
          inv = ::fma(::fma(-hrs * inv, inv, 0.5), inv, inv);
          const double e_cand = (rr2 == 0.0) ? 0.0 : rs * inv;   // e[i+1] = r
          const double sn_n = f * inv, cs_n = g * inv;
          const double g1 = d_hi - p;
          const double rr1 = ::fma(d_i - g1, sn_n, 2.0 * cs_n * b);
          const double p_n = sn_n * rr1;
          const double d_cand = (rr2 == 0.0) ? g1 : g1 + p_n;    // d[i+1]  (tql2: d[i+1] -= p when r == 0)
          const double g_n = ::fma(cs_n, rr1, -b);
          const double rotf = (rr2 == 0.0) ? 0.0 : lv;           // 1: apply this rotation
          de[i + 1] = mk((lv != 0.0) ? d_cand : d_hi, (lv != 0.0) ? e_cand : e_hi);
          const bool on = rotf != 0.0;
          rec[mm - 1 - i] = mk(on ? cs_n : 1.0, on ? sn_n : 0.0);
          sn = on ? sn_n : sn; cs = on ? cs_n : cs; p = on ? p_n : p; g = on ? g_n : g;
          uf += lv - rotf;
          lv = rotf;
          d_hi = d_i; e_hi = e_i; d_i = d_nx; e_i = e_nx;
        }
        underflow = __builtin_amdgcn_readfirstlane((int)(uf != 0.0)) != 0;
      }
      // hand the sweep to the replay: rotations at a 128-byte aligned offset (no cache line is shared by two sweeps, so
      // a replay block that runs concurrently never holds a line that is written later), then the descriptor, then --
      // after a fence -- the published sweep count
      // Publication runs ONE SWEEP BEHIND: the release of sweep q (fence = wait for its stores' acknowledgements, ~1 us when issued right
      // behind them) is issued after the chase of sweep q + 1, when those stores have long landed; the replay is faster than the
      // recurrence anyway, and the last sweep is released by the final store below.
      if (sweeps > 0) {
        __threadfence();
        if (lane == 0) __hip_atomic_store(&S.cnt[0], sweeps, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      }
      for (int k = lane; k < mm - l; k += 64) S.rot[nrot + k] = rec[k];
      if (lane == 0) { S.desc[4 * sweeps] = mm; S.desc[4 * sweeps + 1] = l; S.desc[4 * sweeps + 2] = (int)nrot; S.desc[4 * sweeps + 3] = 0; }
      nrot += (mm - l + 7) & ~7;
      ++sweeps;
      if (underflow) { de[mm].im = 0.0; continue; }
      { const double dl = de[l].re - p; de[l] = mk(dl, g); de[mm].im = 0.0; }
    }
  }
  {
    const double scl = *S.scale;                    // undo the safe scaling (power of two: exact)
    for (int i = lane; i < n; i += 64) w_out[i] = de[i].re / scl;
  }
  __threadfence();                                  // the last sweep's rotations (stored by every lane) before its release below
  if (lane == 0) {
    S.cnt[1] = (int)nrot; S.cnt[2] = overflow;
    __hip_atomic_store(&S.cnt[0], sweeps, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&S.cnt[4], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    if (info) { eigh_set_status(info, overflow ? kEighRotStorage : sweeps); info->cyc_ql = (int)((clock64() - t0) >> 6); info->rotations = (int)nrot; }
  }
}

// Replay of the recorded plane rotations on Z.  One thread per (row, real/imaginary part): the rotations are real, so
// the two parts of a row never mix, and rows are independent.  LDS = true: the workgroup keeps its rows in LDS for the
// whole replay (ReplayLds: bt x n doubles, column-major over the threads: conflict-free), Z is read once and V written once.
// (Streaming the rows through global memory instead stalls on the store acknowledgements -- loads and stores share
// vmcnt on this chip -- ~480 cycles per rotation; it remains as the fallback for n too large for LDS.)
// LIVE = true: the block runs NEXT TO the zungtr and QL-recurrence blocks of the same launch and consumes the sweeps as
// they are published (agent-scope acquire loads of the counters and descriptors, bounded spins).
__device__ __forceinline__ int eigh_spin_until(const int* flag, int want_gt) {   // returns the value read, or INT_MIN on timeout
  for (long long it = 0; it < (1LL << 21); ++it) {
    const int v = __hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
    if (v > want_gt) return v;
    __builtin_amdgcn_s_sleep(16);
  }
  return -2147483647 - 1;
}

template <bool LDS, bool LIVE>
__device__ __forceinline__ void eigh_replay_body(int n, const EighScratch& S, c64* __restrict__ V_out, char* smem_raw, int block,
                                                 int bt, EighInfo* __restrict__ info) {
  const long long t0 = clock64();
  const int tx = threadIdx.x;
  if (tx >= bt) return;                             // (LIVE launch: 1024-thread blocks, the first bt threads work)
  const int gid = block * bt + tx;
  const int n_items = 2 * n;
  const int item = gid < n_items ? gid : n_items - 1;           // surplus lanes shadow the last item (same values, same stores)
  double* Zg = reinterpret_cast<double*>(S.Z) + item;            // element (row, col, part) at Zg[2 n col], item = 2 row + part
  const long long gs = 2 * (long long)n;                         // global column stride in doubles
  double* Zd;
  long long cs;
  bool timeout = false;
  if (LIVE) timeout = eigh_spin_until(&S.cnt[3], 0) < 0;         // Z = Q complete (zungtr block)
  const ReplayLds lds = ReplayLds::of(n, bt, LDS);
  if constexpr (LDS) {
    Zd = reinterpret_cast<double*>(smem_raw + lds.rows) + tx;
    cs = bt;
    for (int c = 0; c < n; ++c) Zd[cs * c] = Zg[gs * c];
  } else {
    Zd = Zg;
    cs = gs;
  }
  const c64* rot = S.rot;
  const int* desc = S.desc;
  // The (c, s) of one sweep are staged in LDS: a direct read per rotation is a dependent L2 round trip (~330 cycles per
  // rotation measured).  Offline they are double buffered (loads of sweep q+1 issued before sweep q is replayed); live,
  // each sweep is fetched when it has been published (the replay is faster than the recurrence that feeds it).
  c64* stage = reinterpret_cast<c64*>(smem_raw + lds.stage);
  const int per_thread = (n + bt - 1) / bt;         // rotations each thread stages per sweep (<= 8 for bt >= n / 8)
  c64 pre[8];
  auto fetch = [&](long long o, int cnt) {          // unconditional loads (clamped): all eight fly together
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = tx + u * bt;
      pre[u] = rot[o + ((u < per_thread && k < cnt) ? k : 0)];
    }
  };
  auto stash = [&](int buf, int cnt) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = tx + u * bt;
      if (u < per_thread && k < cnt) stage[buf * n + k] = pre[u];
    }
  };
  auto block_sync = [&]() {                         // the working threads of the block (one wavefront when bt <= 64)
    if (LIVE) { if (bt > 64) __builtin_amdgcn_s_barrier(); }   // LIVE launches use bt <= 64: a lone wavefront, LDS ops are in order
    else __syncthreads();
  };
  int n_sweeps = LIVE ? 0 : S.cnt[0];
  if (!LIVE && n_sweeps > 0) { fetch(desc[2], desc[0] - desc[1]); stash(0, desc[0] - desc[1]); }
  block_sync();
  for (int q = 0; ; ++q) {
    int mm, lo;
    long long off;
    if (LIVE) {
      if (timeout) break;
      if (q >= n_sweeps) {                          // wait for sweep q, or for the end of the recurrence
        for (long long it = 0; ; ++it) {
          const int done = __hip_atomic_load(&S.cnt[4], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
          n_sweeps = __hip_atomic_load(&S.cnt[0], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
          if (n_sweeps > q || done) break;
          if (it > (1LL << 21)) { timeout = true; break; }
          __builtin_amdgcn_s_sleep(16);
        }
        if (timeout || q >= n_sweeps) break;
      }
      const long long* d8 = reinterpret_cast<const long long*>(desc + 4 * q);
      const long long w0 = __hip_atomic_load(d8, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const long long w1 = __hip_atomic_load(d8 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      mm = (int)(w0 & 0xffffffffLL); lo = (int)(w0 >> 32); off = (int)(w1 & 0xffffffffLL);
      fetch(off, mm - lo);
      stash(q & 1, mm - lo);
      block_sync();
    } else {
      if (q >= n_sweeps) break;
      mm = desc[4 * q]; lo = desc[4 * q + 1]; off = desc[4 * q + 2];
      if (q + 1 < n_sweeps) fetch(desc[4 * q + 6], desc[4 * q + 4] - desc[4 * q + 5]);   // in flight during the replay below
    }
    const int cnt = mm - lo;
    const c64* rec = stage + (q & 1) * n;
    // LDS rows are private, so surplus lanes may replay their shadow copy; in global memory they would race with the
    // owner of the row (a different wavefront) and must sit the sweep out
    if (LDS || gid < n_items) {
      double zhi = Zd[cs * mm];                      // column i+1 of my row, carried between rotations
      int i = mm - 1;
      // full groups of eight rotations: operands of group g+1 are read before group g is computed, nothing conditional
      // inside, and the only loop-carried dependence is one FMA per rotation (zhi)
      double zl[8];
      c64 cg[8];
      if (i - 7 >= lo) {
#pragma unroll
        for (int u = 0; u < 8; ++u) { zl[u] = Zd[cs * (i - u)]; cg[u] = rec[mm - 1 - (i - u)]; }
      }
      while (i - 7 >= lo) {
        double zn[8];
        c64 cn[8];
        const bool next_full = i - 15 >= lo;
        const int ib = next_full ? i - 8 : i;        // (uniform) re-read the same group when no full group follows
#pragma unroll
        for (int u = 0; u < 8; ++u) { zn[u] = Zd[cs * (ib - u)]; cn[u] = rec[mm - 1 - (ib - u)]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          // z[r][i+1] = s z[r][i] + c z[r][i+1];  z[r][i] = c z[r][i] - s z[r][i+1]
          const double czl = cg[u].re * zl[u];
          Zd[cs * (i - u + 1)] = ::fma(cg[u].im, zl[u], cg[u].re * zhi);
          zhi = ::fma(-cg[u].im, zhi, czl);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) { zl[u] = zn[u]; cg[u] = cn[u]; }
        i -= 8;
      }
      for (; i >= lo; --i) {                         // tail (< 8 rotations)
        const c64 c1 = rec[mm - 1 - i];
        const double z1 = Zd[cs * i];
        Zd[cs * (i + 1)] = ::fma(c1.im, z1, c1.re * zhi);
        zhi = ::fma(-c1.im, zhi, c1.re * z1);
      }
      Zd[cs * lo] = zhi;                             // the last carried column
    }
    (void)cnt;
    if (!LIVE && q + 1 < n_sweeps) stash((q + 1) & 1, desc[4 * q + 4] - desc[4 * q + 5]);
    block_sync();
  }
  if (gid < n_items) {
    double* Vd = reinterpret_cast<double*>(V_out) + item;
    for (int c = 0; c < n; ++c) Vd[gs * c] = Zd[cs * c];
  }
  if (gid == 0 && info) { info->cyc_replay = (int)((clock64() - t0) >> 6); if (timeout) eigh_set_status(info, kEighReplayTimeout); }
}

template <bool LDS>
__global__ __launch_bounds__(256) void eigh_replay_kernel(int n, void* scratch, c64* __restrict__ V_out, EighInfo* __restrict__ info,
                                                          const int* __restrict__ ctl) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  if (ctl && ctl[0] == 1) return;
  EighScratch S(scratch, n);
  eigh_replay_body<LDS, false>(n, S, V_out, smem_raw, (int)blockIdx.x, (int)blockDim.x, info);
}

// ---------------------------------------------------------------- Hermitian eigensolver III: the SIGNAL SUBSPACE only (MUSIC, music.m:19-29)
// music.m needs Uan Uan' = I - Us Us' only, with Us the eigenvectors of the L = numDets largest eigenvalues: the full basis the QL pipeline
// above produces (its single-wavefront recurrence was the longest kernel of a CPI) is not needed.  Route (restated in NumPy for CPU-side
// numerics checks: oracle/subspace_music.py):
//   K1  eigh_tridiag_*           as above: Householder reflectors (S.M, S.tau) and the real tridiagonal (S.d, S.e)
//   K2  eigh_bisect_kernel       ALL eigenvalues by Sturm counts (negative pivots of T - x I, dstebz-style pivmin clamp): one wavefront per
//                                eigenvalue, its 64 lanes cut the bracket into 65 parts per round (6 bits; ~9 rounds to eps ||T||)
//   K3, K4  music_subspace_kernel, music_scan_kernel: the signal vectors of the L largest eigenvalues and the scan over them -- music.hip

// Four wavefronts per workgroup = one per SIMD: the count recurrence is a dependent chain of ~12 fp64 instructions per matrix row, and
// a SIMD shared by four such chains runs each at a quarter of the rate (16 waves per workgroup: 70 us at n = 64) while the other CUs idle.
__global__ __launch_bounds__(64 * kBisectWaves) void eigh_bisect_kernel(int n, void* scratch, double* __restrict__ w_out /* [n] ascending */) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  EighScratch S(scratch, n);
  const BisectLds lds = BisectLds::of(n);
  c64* de = reinterpret_cast<c64*>(smem_raw + lds.de);   // (.re = d_i, .im = e_{i-1}^2 with e_{-1} = 0)
  double* sred = reinterpret_cast<double*>(smem_raw + lds.sred);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  double gl = 1.7976931348623157e308, gu = -1.7976931348623157e308, e2m = 0.0;
  for (int i = tid; i < n; i += 64 * kBisectWaves) {     // Gershgorin interval
    const double d = S.d[i];
    const double el = i > 0 ? S.e[i - 1] : 0.0, er = i < n - 1 ? S.e[i] : 0.0;
    de[i] = mk(d, el * el);
    const double rad = fabs(el) + fabs(er);
    gl = fmin(gl, d - rad); gu = fmax(gu, d + rad); e2m = fmax(e2m, el * el);
  }
  gl = wave_min(gl); gu = wave_max(gu); e2m = wave_max(e2m);
  if (lane == 0) { sred[wid] = gl; sred[16 + wid] = gu; sred[32 + wid] = e2m; }
  __syncthreads();
  for (int w = 0; w < kBisectWaves; ++w) { gl = fmin(gl, sred[w]); gu = fmax(gu, sred[16 + w]); e2m = fmax(e2m, sred[32 + w]); }
  const double bnorm = fmax(fabs(gl), fabs(gu));
  const double pivmin = 2.2250738585072014e-308 * fmax(1.0, e2m);
  const double eps = 2.220446049250313e-16;
  const double widen = 2.0 * bnorm * eps * (double)n + 2.0 * pivmin;
  gl -= widen; gu += widen;
  const double tol = 2.0 * eps * bnorm + 2.0 * pivmin;   // absolute: eps ||T|| is what a backward-stable eigensolver delivers
  const int ei = blockIdx.x * kBisectWaves + wid;        // this wavefront's eigenvalue (ascending index)
  if (ei >= n) return;                                   // (wave-uniform; no barrier below)
  double lo = gl, hi = gu;
  for (int it = 0; it < 48; ++it) {                      // (bounded also for NaN input)
    if (!(hi - lo > tol)) break;
    const double x = ::fma(hi - lo, (double)(lane + 1) * (1.0 / 65.0), lo);
    int c = 0;
    double q = 1.0;                                      // q_0 = d_0 - x  (e_{-1}^2 = 0)
    for (int i = 0; i < n; ++i) {
      const c64 v = de[i];                               // (broadcast read)
      q = ::fma(-v.im, rcp_fast(q), v.re - x);
      q = fabs(q) < pivmin ? -pivmin : q;
      c += q < 0.0 ? 1 : 0;
    }
    double nlo = wave_max(c <= ei ? x : lo), nhi = wave_min(c > ei ? x : hi);
    if (nlo > nhi) nlo = nhi = 0.5 * (nlo + nhi);        // (counts within rounding distance of the eigenvalue need not be monotone)
    if (nlo == lo && nhi == hi) break;
    lo = nlo; hi = nhi;
  }
  if (lane == 0) {
    const double w = 0.5 * (lo + hi);
    S.wsc[ei] = w;
    w_out[ei] = w / *S.scale;                            // undo the safe scaling (power of two: exact)
  }
}

}  // namespace isac

// ================================================================= host side
using namespace isac;

// launches of eigh_tridiag_dist_kernel in this process: consecutive ones (of any context) go to consecutive XCDs, so that concurrent reductions of a
// multi-context pipeline do not compete for the workgroup slots of one XCD (each needs its <= 16 workgroups resident together)
static std::atomic<unsigned> td_launches{0};

// Householder tridiagonalisation of H (order n >= 3) into ctx->eig_scratch, on stream st
static int launch_tridiag(isac_ctx* ctx, const c64* d_H, int n, hipStream_t st, EighInfo* info) {
  {
    const void* before = ctx->eig_scratch.p;
    const size_t cap_before = ctx->eig_scratch.cap;
    ISAC_TRY(ensure(ctx, ctx->eig_scratch, EighScratch::bytes(n)));
    if (ctx->eig_scratch.p != before || ctx->eig_scratch.cap != cap_before)                // fresh memory: the step stamps of eigh_tridiag_dist_kernel must not look like stamps of a later epoch
      ISAC_HIP(hipMemsetAsync(ctx->eig_scratch.p, 0, ctx->eig_scratch.cap, st));
  }
  void* gs = ctx->eig_scratch.p;
  if (n <= 64) {       // four waves, two barriers per step, matrix in LDS (the general kernel with its matrix in LDS: 222 us at n = 64; this one ~120)
    ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(eigh_tridiag_small_kernel), (size_t)(112 * 1024)));
    hipLaunchKernelGGL(eigh_tridiag_small_kernel, dim3(1), dim3(64 * kTriWaves), TridiagSmallLds::of(n).bytes, st, d_H, n, gs, info);
  } else {
    static const char* td_env = std::getenv("ISAC_EIG_TRIDIAG_DIST");   // test hook: "0" the one-workgroup kernels for every n; "far" write-through exchange at stride 8; "s1" stride 1
    const bool td_off = td_env && td_env[0] == '0';
    const int td_stride = td_env && td_env[0] == 's' ? std::max(1, std::atoi(td_env + 1)) : 8, td_far = td_env && td_env[0] == 'f';
    const bool dist = n <= kTdMaxN && !td_off;
    if (dist) {
      if (((++ctx->eig_epoch) & 0xFFFFF) == 0) {                                      // the 20-bit epoch of the tags wraps: start over from a clean area
        ++ctx->eig_epoch;
        ISAC_HIP(hipMemsetAsync(ctx->eig_scratch.p, 0, EighScratch::kXchBytes, st));
      }
      // every 8th workgroup of the grid works (the others return at once): the dispatcher deals workgroups round-robin to the 8 XCDs, so the working ones share
      // an L2 and the exchange can stay in it -- verified by the kernel (XCC ids in its first exchange), never assumed
      static const bool force_to = std::getenv("ISAC_EIG_FORCE_TRIDIAG_TIMEOUT") != nullptr;   // test hook: every distributed reduction reports a time-out
      ISAC_HIP(hipMemsetAsync(&info->sticky, 0, sizeof(int), st));                        // the sticky time-out word (the one-workgroup kernels clear it themselves)
      hipLaunchKernelGGL(eigh_tridiag_dist_kernel, dim3((unsigned)(((n + 15) / 16) * td_stride)), dim3(256), 0, st, d_H, n, gs, info,
                         (unsigned)((ctx->eig_epoch & 0xFFFFF) << 12), td_stride, (int)(td_launches.fetch_add(1) % (unsigned)td_stride), td_far, force_to ? 1 : 0);
    } else {
      const size_t ldsf = TridiagFusedLds::of(n).bytes;
      ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(eigh_tridiag_fused_kernel), ldsf));
      hipLaunchKernelGGL(eigh_tridiag_fused_kernel, dim3(1), dim3(1024), ldsf, st, d_H, n, gs, info);
    }
  }
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}

// the recorded rotations applied to Z by a launch of its own (rows in LDS while they fit)
static int launch_replay_offline(isac_ctx* ctx, int n, hipStream_t st, EighInfo* info, const int* ctl) {
  void* gs = ctx->eig_scratch.p;
  const ReplayLds rl = ReplayLds::of(n);
  if (rl.rows_in_lds) {
    ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(eigh_replay_kernel<true>), rl.bytes));
    hipLaunchKernelGGL(eigh_replay_kernel<true>, dim3((unsigned)((2 * n + rl.bt - 1) / rl.bt)), dim3(rl.bt), rl.bytes, st, n, gs, (c64*)ctx->eig_v.p, info, ctl);
  } else {
    hipLaunchKernelGGL(eigh_replay_kernel<false>, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), ReplayLds::of(n, 256, false).bytes, st, n, gs, (c64*)ctx->eig_v.p, info, ctl);
  }
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}

// zungtr || QL recurrence || replay on the tridiagonal form in ctx->eig_scratch -> ctx->eig_w / eig_v.  `ctl` (device, may be null): the
// kernels return at once when ctl[0] == 1 (music_subspace_kernel has already delivered what MUSIC needs).
int isac_eigh_ql_dev(isac_ctx* ctx, int n, hipStream_t st, const int* ctl, bool allow_live) {
  void* gs = ctx->eig_scratch.p;
  EighInfo* info = eig_info(ctx, n);
  // (forcing the zungtr block and the lone recurrence wavefront onto different CUs with an oversized LDS request made no
  // difference to the recurrence -- 345 vs 350 cycles per rotation at the time -- and cost CU capacity in pipelined runs)
  const FormqQlLds ql = FormqQlLds::of(n);
  const ReplayLds rl = ReplayLds::of(n);
  // Replay blocks ride along with zungtr and the recurrence (they spin on flags of the same launch: co-resident workgroups are a speed
  // assumption, a bounded spin turns a violation into an error) -- except when this is the in-stream fallback of the subspace route
  // (ctl != null): there the replay is its own launch behind the recurrence, so the rare large-numDets CPI cannot fail on a spin time-out
  const bool live = rl.rows_in_lds && ctl == nullptr && allow_live;
  const int n_replay = (2 * n + rl.bt - 1) / rl.bt;
  ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(eigh_formq_ql_kernel), (size_t)(160 * 1024)));
  // (as the in-stream fallback it almost always returns at its first instruction: 256 threads then -- a 1024-thread workgroup of ~110 VGPRs needs a
  // whole CU to itself and sat 90-140 us in its queue while the next CPI's echo kernel held every CU with two workgroups, profiles/r03_device_timeline.txt)
  hipLaunchKernelGGL(eigh_formq_ql_kernel, dim3(live ? 2 + n_replay : 2), dim3(ctl ? 256 : 1024), live ? ql.bytes_live : ql.bytes, st, n, gs,
                     (double*)ctx->eig_w.p, info, (c64*)ctx->eig_v.p, rl.bt, ctl);
  ISAC_HIP(hipGetLastError());
  if (!live) ISAC_TRY(launch_replay_offline(ctx, n, st, info, ctl));
  return ISAC_OK;
}

// Recovery of a CPI whose LIVE replay blocks gave up waiting (kEighReplayTimeout; co-resident workgroups of one launch are a speed assumption
// HIP does not guarantee): the zungtr result Z and every recorded rotation are intact once the launch has finished -- the recurrence and
// zungtr blocks never wait for the replay blocks -- so the eigenvectors are formed by the offline replay, as on the fallback route.
int isac_eigh_replay_recover(isac_ctx* ctx, int n, hipStream_t st) {
  if (!st) st = ctx->stream;
  EighInfo* info = eig_info(ctx, n);
  ISAC_HIP(hipMemsetAsync(&info->status, 0, sizeof(int), st));                 // the time-out mark; the replay below cannot time out
  return launch_replay_offline(ctx, n, st, info, nullptr);
}

// first half: reflectors + all eigenvalues (ascending, ctx->eig_w); independent of numDets
int isac_music_tridiag_bisect_dev(isac_ctx* ctx, const c64* d_H, int A, hipStream_t st) {
  if (!st) st = ctx->stream;
  const int n = A;
  ISAC_TRY(ensure_eig_out(ctx, A));
  ISAC_TRY(ensure(ctx, ctx->misc, 512));
  ISAC_TRY(launch_tridiag(ctx, d_H, n, st, eig_info(ctx, A)));
  hipLaunchKernelGGL(eigh_bisect_kernel, dim3((unsigned)((n + kBisectWaves - 1) / kBisectWaves)), dim3(64 * kBisectWaves), BisectLds::of(n).bytes, st, n, ctx->eig_scratch.p,
                     (double*)ctx->eig_w.p);
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}

// device eig: H [A x A] (device) -> ctx->eig_w [A], ctx->eig_v [A x A] (unsorted)
// live_replay = false: the recorded rotations are applied by a launch of their own behind the recurrence instead of by blocks that spin on its progress inside the
// same launch -- for callers that cannot run the time-out recovery (isac_eigh_replay_recover) before the result is consumed on the device: the fft2D pipeline
int isac_eigh_dev(isac_ctx* ctx, const c64* d_H, int A, hipStream_t st, bool live_replay) {
  if (!st) st = ctx->stream;
  if (A > 1024) return fail(ctx, ISAC_ERR_UNSUPPORTED, "device eigensolver supports up to 1024 antennas");
  // measured host-call times (tools/_eig_sizes.py): Jacobi 0.10 / 0.16 / 0.26 / 0.35 / 0.78 / 1.41 ms at A = 8 / 16 / 24 / 32 / 48 /
  // 64, the tridiagonal pipeline 0.10 / 0.17 / 0.24 / 0.33 / 0.57 / 0.86 ms: Jacobi up to 16 antennas, the pipeline beyond
  ISAC_TRY(ensure_eig_out(ctx, A));
  EighInfo* info = eig_info(ctx, A);
  if (A > kJacobiMaxA) {
    ISAC_TRY(launch_tridiag(ctx, d_H, A, st, info));
    return isac_eigh_ql_dev(ctx, A, st, nullptr, live_replay);
  }
  const size_t lds = JacobiLds::of(A).bytes;
  ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(jacobi_eigh_kernel), lds));
  hipLaunchKernelGGL(jacobi_eigh_kernel, dim3(1), dim3(1024), lds, st, d_H, A, 40, (double*)ctx->eig_w.p, (c64*)ctx->eig_v.p, info);
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}
