// Per-target list of fft2D (gfx950 only): isac_fft2d_get_targets joins what the last completed fft2D left on the context -- the range rows ymid [rows x L x A], the power
// window pwin [nr x nc x A] and the per-antenna CFAR lists -- into paired (range, velocity, azimuth) entries.  Project-defined (include/isac_targets.h):
//   1  S = sum over antennas of the power window (fp64, ascending antenna order from 0.0); hits = antennas whose CFAR list holds the cell
//   2  target cell = CUT cell with hits >= 1 and S strictly above all 8 neighbours
//   3  snapshot x[a] = rdm(r, c, a): a single-bin DFT over the L symbols of row r (the expression of doppler_pow_kernel before the modulus)
//   4  azimuth = first arg-max of the Bartlett scan |a_i' x|^2 over MUSIC's ULA grid (same sind table, same steering expression as music_scan_kernel)
//   5  host: sort by S descending, ties by ascending column-major index; rng / vel as fft2D.m:77-82
// K1 target_hits_kernel scatters the lists into a zeroed hits map (its own launch: the map must be complete before any cell is tested), K2 target_cells_kernel sums, tests and
// compacts, K3 target_doa_kernel forms snapshot and azimuth of every selected cell.  All three are latency-bound (a few MB at the bench shape) and off the timed path.
// isac_fft2d_get_targets_upa (include/isac_targets_upa.h) is the same list for a uniform planar array: steps 1, 2, 3 and 5 are the same host function and the same device code
// (select_cells, K1, K2, target_snapshot), and step 4 becomes
//   4' (azimuth, elevation) = first arg-max of |a_j' x|^2 over the [eSteps x aSteps] grid of music.m:36-53, j = e + eSteps a (the table and steering element of doa2d.hip)
// K4 target_snap_kernel writes the snapshots [A x n]; K5 target_scan2d_kernel, one workgroup per tile of PT scan points, forms the steering tile in LDS ONCE and runs every
// snapshot over it -- eSteps aSteps A sincos in all, not that many per target -- leaving one (max, lowest j) per (tile, target); K6 target_scan2d_reduce_kernel joins each
// target's partials in ascending tile order.  No floating-point atomics, no order that depends on arrival: the result is a function of the snapshots alone.
// isac_fft2d_beam_detect (include/isac_beams.h, beams.hip) runs steps 1, 2 and 5 on its beam planes and per-beam lists through target_cells_of_planes: the same host function
// (select_cells) and K1, K2 with the map M = the maximum over the planes in place of their sum (target_cells_kernel<true>); step 3's chain is csrc/rdm_cell.hpp, shared with it.
// isac_fft2d_refine_targets (include/isac_refine.h, refine.hip) runs step 4 / 4' on its refined snapshots through target_scan_snapshots: K3' target_azi_kernel is phase 2 of
// K3 by itself (one device function, target_bartlett_ula, serves both), K5 and K6 are launched by the one host function (enqueue_scan2d) the UPA list launches them with.
#include <algorithm>
#include <numeric>

#include "isac_internal.hpp"
#include "beam_cell.hpp"
#include "rdm_cell.hpp"
#include "upa_steer.hpp"

namespace isac {

// ---------------------------------------------------------------- K1: hits[r, c] = number of antennas whose CFAR list holds (r, c)
// Integer atomicAdd into a zeroed map: the result does not depend on the order the lists are visited in.
__global__ __launch_bounds__(256) void target_hits_kernel(const int* __restrict__ det_cut /* [A x cap] CUT ordinals */, const int* __restrict__ det_cnt /* [A] */, int cap,
                                                          int n_cut_rows, int n_cut, int hr, int hc, int nr, int* __restrict__ hits /* [nr x nc] */) {
  const int a = blockIdx.y;
  const int n = min(det_cnt[a], cap);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int ord = det_cut[(long long)a * cap + i];
    if ((unsigned)ord >= (unsigned)n_cut) continue;                       // (never for a list cfar_*_kernel wrote)
    const int cr = ord % n_cut_rows, cc = ord / n_cut_rows;
    atomicAdd(&hits[(cr + hr) + nr * (cc + hc)], 1);
  }
}

// ---------------------------------------------------------------- K2: integrated map, local-maximum test, compaction
// One workgroup per kCellR x kCellC tile of CUT cells.  One thread per cell of the tile + a one-cell rim sums the A planes of the power window (stride nr * nc: lanes along a
// window column read consecutive doubles); the sums stay in LDS, so a neighbour's S is the very value that neighbour is tested with.  Candidates leave through a wave ballot
// and one atomicAdd per wave; their order is whatever the waves arrive in -- the host sorts.
constexpr int kCellR = 32, kCellC = 8;

// MAX (isac_fft2d_beam_detect, whose planes are beams): the map is M = the maximum over the planes instead of their sum, and each candidate carries the plane of its
// maximum -- the first one in ascending plane order; a NaN never wins, and M is NaN only where every plane is.
template <bool MAX>
__global__ __launch_bounds__(kCellR * kCellC) void target_cells_kernel(const double* __restrict__ pwin /* [nr x nc x A] */, int nr, int nc, int A, int hr, int hc,
                                                                       int n_cut_rows, int n_cut_cols, const int* __restrict__ hits,
                                                                       unsigned* __restrict__ count, int* __restrict__ cand_cut /* [n_cut] CUT ordinal */,
                                                                       int* __restrict__ cand_hits, double* __restrict__ cand_s, int* __restrict__ cand_plane /* MAX only */) {
  constexpr int SR = kCellR + 2, SC = kCellC + 2;
  __shared__ double s_s[SC * SR];                                         // column-major tile + rim
  __shared__ int s_plane[MAX ? SC * SR : 1];
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * kCellR, c0 = blockIdx.y * kCellC;           // first CUT row / column of the tile (0-based)
  const long long plane = (long long)nr * nc;
  for (int i = tid; i < SR * SC; i += kCellR * kCellC) {
    const int lr = i % SR, lc = i / SR;
    const int wr = hr + r0 + lr - 1, wc = hc + c0 + lc - 1;               // window coordinates (hr, hc >= 1: never negative)
    double s = __builtin_nan("");                                          // past the window (a tile that overhangs the zone): never a valid cell's neighbour
    if (wr < nr && wc < nc) {
      const double* p = pwin + wr + (long long)nr * wc;
      if constexpr (MAX) {
        int best = 0;
        s = planes_first_max(p, plane, A, &best);                         // beam_cell.hpp: strictly greater, the first maximum stays
        s_plane[lc * SR + lr] = best;
      } else {
        s = 0.0;
        for (int a = 0; a < A; ++a) s = __dadd_rn(s, p[plane * a]);       // ascending antenna order, from 0.0
      }
    }
    s_s[lc * SR + lr] = s;
  }
  __syncthreads();
  const int lr = tid % kCellR, lc = tid / kCellR;
  const int cr = r0 + lr, cc = c0 + lc;
  bool tgt = false;
  int h = 0;
  const double* q = s_s + (lc + 1) * SR + (lr + 1);
  const double v = *q;
  if (cr < n_cut_rows && cc < n_cut_cols) {
    h = hits[(hr + cr) + nr * (hc + cc)];
    // strictly greater than all 8 neighbours: a plateau gives no target, NaN (on either side) compares false
    tgt = h >= 1 && v > q[-SR - 1] && v > q[-SR] && v > q[-SR + 1] && v > q[-1] && v > q[1] && v > q[SR - 1] && v > q[SR] && v > q[SR + 1];
  }
  const unsigned long long mask = __ballot(tgt);
  const int lane = tid & 63;
  unsigned base = 0;
  if (lane == 0 && mask) base = atomicAdd(count, (unsigned)__popcll(mask));
  base = __shfl(base, 0);
  if (tgt) {
    const unsigned pos = base + (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
    if (pos < (unsigned)(n_cut_rows * n_cut_cols)) {                      // (a cell is counted once: always true)
      cand_cut[pos] = cr + n_cut_rows * cc;
      cand_hits[pos] = h;
      cand_s[pos] = v;
      if constexpr (MAX) cand_plane[pos] = s_plane[(lc + 1) * SR + (lr + 1)];
    }
  }
}

// ---------------------------------------------------------------- K3: array snapshot + Bartlett azimuth of one target cell per workgroup
// Phase 1: x[a] = rdm(r, c, a) in LDS.  Four lanes share an antenna, each runs doppler_pow_kernel's multiply-add chain over a quarter of the symbols; the quarters are
// added pairwise ((q0 + q1) + (q2 + q3): fp addition commutes, so all four lanes hold the same bits).
// Phase 2: one lane per scan angle reads x[m] from LDS -- every lane the same address, a broadcast: no bank conflict whatever the c64 layout -- and forms
// B = |sum_m conj(a[m]) x[m]|^2; angles with bitwise equal sind (mirror twins) run the same instructions on the same operands.  Arg-max: each lane keeps its first
// maximum in ascending angle order, then a fixed tree on (value, lowest index).

// Phase 1 (step 3) for a workgroup of 256 threads, shared by K3 and K4: s_x[0 .. A) = the snapshot of cell (row, c), visible to every thread on return.
__device__ __forceinline__ void target_snapshot(const c64* __restrict__ ymid /* [n_rows x L x A] */, int n_rows, int L, int A, int n_fft,
                                                const c64* __restrict__ tw_d /* e^{-2 pi j m / n_fft} */, double sqrt_nfft, int row /* window row, 0-based */,
                                                int c /* rdm column, 0-based */, c64* s_x /* LDS [A] */) {
  const int tid = threadIdx.x;
  const int kbin = rdm_bin_of_column(c, n_fft);
  for (int base = 0; base < 4 * A; base += 256) {                         // (256 = 64 quads: a quad is inside one wave and all of it active or none)
    const int a = (base + tid) >> 2, part = tid & 3;
    c64 acc = mk(0.0, 0.0);
    if (a < A) acc = rdm_cell_quarter(ymid + row + (long long)n_rows * L * a, n_rows, L, n_fft, kbin, part, tw_d);   // the chain of a cell: rdm_cell.hpp
    acc.re += __shfl_xor(acc.re, 1); acc.im += __shfl_xor(acc.im, 1);
    acc.re += __shfl_xor(acc.re, 2); acc.im += __shfl_xor(acc.im, 2);
    if (a < A && part == 0) s_x[a] = rdm_cell_scale(acc, sqrt_nfft);
  }
  __syncthreads();
}

// Phase 2 (step 4) for a workgroup of 256 threads, shared by K3 and K3': *out_bin = the first arg-max of the scan of the snapshot s_x (LDS [A], visible to every thread).
__device__ __forceinline__ void target_bartlett_ula(const c64* s_x, int A, const double* __restrict__ sind_tab, int n_steps, double d_ratio,
                                                    double* s_val /* LDS [256] */, int* s_idx /* LDS [256] */, int* __restrict__ out_bin) {
  const int tid = threadIdx.x;
  double best = -1.0;                                                     // B >= 0; NaN never wins
  int best_i = 0x7fffffff;
  for (int i = tid; i < n_steps; i += 256) {
    const double sd = sind_tab[i];
    c64 y = mk(0.0, 0.0);
    for (int m = 0; m < A; ++m) {
      double arg = ((-2.0 * M_PI) * (double)m) * d_ratio;                 // exp(-2j*pi*m*d*sind(ph)), left to right as music_scan_kernel (music.m:82)
      arg = arg * sd;
      double s, co;
      sincos(arg, &s, &co);
      y = fma(mk(co, -s), s_x[m], y);                                     // conj(a[m]) x[m]
    }
    const double b = y.re * y.re + y.im * y.im;
    if (b > best) { best = b; best_i = i; }
  }
  s_val[tid] = best;
  s_idx[tid] = best_i;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      const double v2 = s_val[tid + o];
      const int i2 = s_idx[tid + o];
      if (v2 > s_val[tid] || (v2 == s_val[tid] && i2 < s_idx[tid])) { s_val[tid] = v2; s_idx[tid] = i2; }
    }
    __syncthreads();
  }
  if (tid == 0) *out_bin = s_idx[0] == 0x7fffffff ? 0 : s_idx[0];
}

__global__ __launch_bounds__(256) void target_doa_kernel(const c64* __restrict__ ymid /* [n_rows x L x A] */, int n_rows, int L, int A, int n_fft,
                                                         const c64* __restrict__ tw_d /* e^{-2 pi j m / n_fft} */, double sqrt_nfft,
                                                         const int* __restrict__ cell_row /* window row, 0-based */, const int* __restrict__ cell_col /* rdm column, 0-based */,
                                                         const double* __restrict__ sind_tab, int n_steps, double d_ratio,
                                                         int* __restrict__ azi_bin /* [n] */, c64* __restrict__ snap /* [A x n] */) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  c64* s_x = reinterpret_cast<c64*>(smem_raw);                            // [A]
  __shared__ double s_val[256];
  __shared__ int s_idx[256];
  const int tid = threadIdx.x, t = blockIdx.x;
  target_snapshot(ymid, n_rows, L, A, n_fft, tw_d, sqrt_nfft, cell_row[t], cell_col[t], s_x);
  for (int a = tid; a < A; a += 256) snap[a + (long long)A * t] = s_x[a];
  target_bartlett_ula(s_x, A, sind_tab, n_steps, d_ratio, s_val, s_idx, azi_bin + t);
}

// ---------------------------------------------------------------- K3': phase 2 of K3 on snapshots that are already there (isac_fft2d_refine_targets: the refined snapshots)
__global__ __launch_bounds__(256) void target_azi_kernel(const c64* __restrict__ snap /* [A x n] */, int A, const double* __restrict__ sind_tab, int n_steps, double d_ratio,
                                                         int* __restrict__ azi_bin /* [n] */) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  c64* s_x = reinterpret_cast<c64*>(smem_raw);                            // [A]
  __shared__ double s_val[256];
  __shared__ int s_idx[256];
  const int t = blockIdx.x;
  for (int a = threadIdx.x; a < A; a += 256) s_x[a] = snap[a + (long long)A * t];
  __syncthreads();
  target_bartlett_ula(s_x, A, sind_tab, n_steps, d_ratio, s_val, s_idx, azi_bin + t);
}

// ---------------------------------------------------------------- K4: array snapshot of one target cell per workgroup (the UPA list: phase 1 of K3 alone)
__global__ __launch_bounds__(256) void target_snap_kernel(const c64* __restrict__ ymid /* [n_rows x L x A] */, int n_rows, int L, int A, int n_fft,
                                                          const c64* __restrict__ tw_d, double sqrt_nfft, const int* __restrict__ cell_row,
                                                          const int* __restrict__ cell_col, c64* __restrict__ snap /* [A x n] */) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  c64* s_x = reinterpret_cast<c64*>(smem_raw);                            // [A]
  const int t = blockIdx.x;
  target_snapshot(ymid, n_rows, L, A, n_fft, tw_d, sqrt_nfft, cell_row[t], cell_col[t], s_x);
  for (int a = threadIdx.x; a < A; a += 256) snap[a + (long long)A * t] = s_x[a];
}

// ---------------------------------------------------------------- K5: 2-D Bartlett scan of every snapshot over one tile of PT scan points per workgroup
// The tile conj(a_j[r]), [A x PT] c64 (64 KB at PT = 64 / 32 / 16 for A = 64 / 128 / 256; a row of PT consecutive c64 per element, so the PT lanes of a point group read
// consecutive 16-byte words), is formed once with doa2d_scan_kernel's steering element and then serves all n snapshots.  Thread (p, g) = (tid % PT, tid / PT): point j0 + p,
// snapshots g, g + G, ... (G = 256 / PT).  x[r] of a snapshot is one address for the PT lanes of a group: a broadcast load out of L2 (n <= 1024 snapshots, at most 4 MB).
// EVERY (point, snapshot) value is the same chain -- y = fma(conj(a[r]), x[r], y) over r ascending from 0, then re^2 + im^2 -- wherever the point sits in its tile: equal
// steering vectors (the mirror twins) give bitwise equal values.  The arg-max over the tile is a butterfly on (value, lowest j) across the group's PT lanes (PT divides 64: a
// group never straddles a wave); the operation is associative and commutative, so the butterfly's order does not matter.  Tail points (j >= eSteps aSteps) take part as
// (-1, INT_MAX) and never win; neither does a NaN.
template <int PT>
__global__ __launch_bounds__(256) void target_scan2d_kernel(const double* __restrict__ tab, int eS, int aS, int nV, int nH, const c64* __restrict__ snap /* [A x n] */, int n,
                                                            double* __restrict__ part_val /* [tiles x n] */, int* __restrict__ part_idx /* [tiles x n] */) {
  constexpr int G = 256 / PT;
  static_assert(64 % PT == 0, "a point group must lie inside one wave");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  c64* s_a = reinterpret_cast<c64*>(smem_raw);                            // [A][PT], conjugated
  const int A = nV * nH, n_pts = eS * aS;
  const int tid = threadIdx.x, j0 = blockIdx.x * PT;
  for (int t = tid; t < A * PT; t += 256) {
    const int p = t % PT, r = t / PT;
    s_a[t] = conj(upa_steer(tab, eS, aS, nH, min(j0 + p, n_pts - 1), r));   // (tail points repeat the last one; they never win)
  }
  __syncthreads();
  const int p = tid % PT, g = tid / PT, j = j0 + p;
  for (int t0 = 0; t0 < n; t0 += G) {                                     // (uniform trip count: every lane takes part in the butterfly)
    const int t = t0 + g;
    const c64* x = snap + (long long)A * min(t, n - 1);
    c64 y = mk(0.0, 0.0);
    for (int r = 0; r < A; ++r) y = fma(s_a[r * PT + p], x[r], y);        // conj(a[r]) x[r]
    const double b = y.re * y.re + y.im * y.im;
    double best = -1.0;                                                   // B >= 0; NaN never wins
    int best_j = 0x7fffffff;
    if (j < n_pts && b > best) { best = b; best_j = j; }
    for (int o = PT / 2; o > 0; o >>= 1) {
      const double v2 = __shfl_xor(best, o);
      const int j2 = __shfl_xor(best_j, o);
      if (v2 > best || (v2 == best && j2 < best_j)) { best = v2; best_j = j2; }
    }
    if (p == 0 && t < n) {
      part_val[(size_t)blockIdx.x * n + t] = best;
      part_idx[(size_t)blockIdx.x * n + t] = best_j;
    }
  }
}

// ---------------------------------------------------------------- K6: each target's partials joined in ascending tile order -> the first arg-max over the whole grid
__global__ __launch_bounds__(256) void target_scan2d_reduce_kernel(const double* __restrict__ part_val, const int* __restrict__ part_idx, int n_tiles, int n,
                                                                   int* __restrict__ best_bin /* [n]: j = e + eSteps a */) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  double best = -1.0;
  int best_j = 0x7fffffff;
  for (int tile = 0; tile < n_tiles; ++tile) {                            // (lanes along t: consecutive words)
    const double v2 = part_val[(size_t)tile * n + t];
    const int j2 = part_idx[(size_t)tile * n + t];
    if (v2 > best || (v2 == best && j2 < best_j)) { best = v2; best_j = j2; }
  }
  best_bin[t] = best_j == 0x7fffffff ? 0 : best_j;
}

}  // namespace isac

// ================================================================= host side
using namespace isac;

namespace {

// What both entry points ask first: the caller's arguments, and a completed fft2D whose device state is still the one it left.  who: the entry point, for the message.
int cpi_ready(isac_ctx* ctx, const char* who, const isac_target_list* out, const isac_c64* snapshots, int32_t cap_snap) {
  if (!out || (snapshots && cap_snap < 0)) return fail(ctx, ISAC_ERR_INVALID_ARG, "NULL argument");
  if (!ctx->last.valid || ctx->tgt.state != Fft2dCpi::kCollected)
    return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": no completed fft2D on this context whose range rows, power window and detection lists are still on the device");
  return ISAC_OK;
}

// The selected cells on the device: n of them (0: none, the list is complete), [window row | rdm column] at d + off_sel; room for a scan bin per target at d + off_bin and
// for the snapshots [A x n] at d + off_snap (d = ctx->tgt_scratch)
struct SelectedCells {
  int n = 0;
  char* d = nullptr;
  size_t off_sel = 0, off_bin = 0, off_snap = 0;
};

// Steps 1, 2 and 5 of both lists -- they do not know the array type: K1, K2, the sort, the ISAC_MAX_TARGETS cut, every field of *out but azi and n_targets, and (sc != NULL)
// the upload of the selected cells for the kernels of steps 3 and 4.  src: the planes and per-plane lists the cells are taken from -- the power window and the CFAR lists of
// the CPI for the two lists, the beam planes and per-beam lists for isac_fft2d_beam_detect (take_max: the map is the maximum over the planes, best_plane[i] its first plane).
int select_cells(isac_ctx* ctx, const char* who, const PlaneCells& src, isac_target_list* out, const isac_c64* snapshots, int32_t cap_snap, SelectedCells* sc) {
  const Fft2dCpi& ts = ctx->tgt;
  const isac_est_params& ep = ts.ep;
  const CutWindow& w = ts.win;
  const int hr = w.hr, hc = w.hc;
  ISAC_TRY(needs_halo(ctx, who));
  const int A = ts.A, nr = w.nr, nc = w.nc, n_cut_rows = w.n_cut_rows, n_cut_cols = w.n_cut_cols, n_cut = (int)w.n_cut();
  if (sc) *sc = SelectedCells{};
  std::memset(out, 0, sizeof(*out));
  // one scratch block: [hits nr x nc | count (16 ints)] zeroed, then the candidate lists, the selected cells and their results
  const size_t n_map = (size_t)nr * nc;
  const size_t off_cnt = sizeof(int) * n_map, off_ccut = off_cnt + 64, off_chit = off_ccut + sizeof(int) * (size_t)n_cut;
  const size_t off_cpl = off_chit + sizeof(int) * (size_t)n_cut;          // the candidates' planes: take_max only
  const size_t off_cs = (off_cpl + (src.take_max ? sizeof(int) * (size_t)n_cut : 0) + 15) & ~(size_t)15, off_sel = off_cs + sizeof(double) * (size_t)n_cut;
  const size_t off_azi = off_sel + sizeof(int) * 2 * ISAC_MAX_TARGETS, off_snap = (off_azi + sizeof(int) * ISAC_MAX_TARGETS + 15) & ~(size_t)15;
  ISAC_TRY(ensure(ctx, *src.scratch, off_snap + (sc ? sizeof(c64) * (size_t)A * ISAC_MAX_TARGETS : 0)));
  char* d = (char*)src.scratch->p;
  ISAC_HIP(hipMemsetAsync(d, 0, off_ccut, ctx->stream));
  hipLaunchKernelGGL(target_hits_kernel, dim3(std::min(cdiv(src.cap, 256), 8u), src.n_planes), dim3(256), 0, ctx->stream, src.det_cut, src.det_cnt, src.cap,
                     n_cut_rows, n_cut, hr, hc, nr, (int*)d);
  ISAC_HIP(hipGetLastError());
  auto cells = src.take_max ? target_cells_kernel<true> : target_cells_kernel<false>;
  hipLaunchKernelGGL(cells, dim3(cdiv(n_cut_rows, kCellR), cdiv(n_cut_cols, kCellC)), dim3(kCellR * kCellC), 0, ctx->stream, src.planes, nr, nc,
                     src.n_planes, hr, hc, n_cut_rows, n_cut_cols, (const int*)d, (unsigned*)(d + off_cnt), (int*)(d + off_ccut), (int*)(d + off_chit), (double*)(d + off_cs),
                     src.take_max ? (int*)(d + off_cpl) : (int*)nullptr);
  ISAC_HIP(hipGetLastError());
  unsigned count = 0;
  ISAC_TRY(copy_d2h(ctx, &count, d + off_cnt, sizeof(count)));
  if (count > (unsigned)n_cut) return fail(ctx, ISAC_ERR_HIP, "internal: more target cells than CUTs");
  const int n_total = (int)count;
  out->n_total = n_total;
  if (n_total == 0) return ISAC_OK;
  std::vector<int> ccut((size_t)n_total), chit((size_t)n_total), cpl;
  std::vector<double> cs((size_t)n_total);
  ISAC_TRY(copy_d2h(ctx, ccut.data(), d + off_ccut, sizeof(int) * (size_t)n_total));
  ISAC_TRY(copy_d2h(ctx, chit.data(), d + off_chit, sizeof(int) * (size_t)n_total));
  ISAC_TRY(copy_d2h(ctx, cs.data(), d + off_cs, sizeof(double) * (size_t)n_total));
  if (src.take_max) {
    cpl.resize((size_t)n_total);
    ISAC_TRY(copy_d2h(ctx, cpl.data(), d + off_cpl, sizeof(int) * (size_t)n_total));
  }
  // S descending, ties by ascending column-major index r + nIFFT (c - 1) -- the order of the CUT ordinal cr + n_cut_rows cc (column first, then row)
  std::vector<int> order((size_t)n_total);
  std::iota(order.begin(), order.end(), 0);
  std::sort(order.begin(), order.end(), [&](int p, int q) {
    if (cs[(size_t)p] != cs[(size_t)q]) return cs[(size_t)p] > cs[(size_t)q];
    return ccut[(size_t)p] < ccut[(size_t)q];
  });
  const int n = std::min(n_total, (int)ISAC_MAX_TARGETS);
  if (snapshots && n > cap_snap) return fail(ctx, ISAC_ERR_CAPACITY, std::string(who) + ": more targets than snapshot columns");
  std::vector<int> sel((size_t)2 * n);                                    // [window row | rdm column], 0-based
  for (int i = 0; i < n; ++i) {
    const int o = order[(size_t)i];
    const CutWindow::RowCol rc = w.row_col_of(ccut[(size_t)o]);           // 1-based
    out->row[i] = rc.row;
    out->col[i] = rc.col;
    out->hits[i] = chit[(size_t)o];
    out->power[i] = cs[(size_t)o];
    out->rng[i] = CutWindow::range_of(rc.row, ep);
    out->vel[i] = CutWindow::velocity_of(rc.col, ep);
    if (src.take_max) src.best_plane[i] = cpl[(size_t)o];
    sel[(size_t)i] = rc.row - w.first_row;
    sel[(size_t)n + i] = rc.col - 1;
  }
  if (!sc) return ISAC_OK;
  ISAC_TRY(stage_upload(ctx, d + off_sel, sel.data(), sizeof(int) * sel.size()));
  *sc = SelectedCells{n, d, off_sel, off_azi, off_snap};
  return ISAC_OK;
}

// the planes and lists of the two per-target lists: the CPI's own
PlaneCells cpi_cells(isac_ctx* ctx) {
  return PlaneCells{(const double*)ctx->pwin.p, ctx->tgt.A, (const int*)ctx->det_cut.p, (const int*)ctx->det_cnt.p, ctx->tgt.cap, false, &ctx->tgt_scratch, nullptr};
}

// The scan bins of the n selected cells and, when asked for, their snapshots: complete when it returns
int fetch_bins(isac_ctx* ctx, const SelectedCells& sc, int A, std::vector<int>& bins, isac_c64* snapshots) {
  bins.resize((size_t)sc.n);
  ISAC_TRY(copy_d2h(ctx, bins.data(), sc.d + sc.off_bin, sizeof(int) * (size_t)sc.n));
  if (snapshots) ISAC_TRY(copy_d2h(ctx, snapshots, sc.d + sc.off_snap, sizeof(c64) * (size_t)A * sc.n));
  return ISAC_OK;
}

// Step 4' on the device: K5 + K6 over n snapshots [A x n] -> d_bin [n], j = e + eSteps a.  Enqueued on the context's stream; the partials live in ctx->tgt_part.
int enqueue_scan2d(isac_ctx* ctx, const isac_est_params& ep, int A, const double* d_tab, int e_steps, int a_steps, const c64* d_snap, int n, int* d_bin) {
  const int pt = A <= 64 ? 64 : A <= 128 ? 32 : 16;                       // the steering tile [A x pt] c64 fits 64 KB of LDS
  const long long n_pts = (long long)e_steps * a_steps;
  const unsigned n_tiles = cdiv(n_pts, pt);
  ISAC_TRY(ensure(ctx, ctx->tgt_part, (sizeof(double) + sizeof(int)) * (size_t)n_tiles * n));
  double* part_val = (double*)ctx->tgt_part.p;
  int* part_idx = (int*)(part_val + (size_t)n_tiles * n);
#define ISAC_TARGET_SCAN2D(PT_)                                                                                                                          \
  do {                                                                                                                                                   \
    const size_t lds = sizeof(c64) * (size_t)A * PT_;                                                                                                    \
    ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(target_scan2d_kernel<PT_>), lds));                                                             \
    hipLaunchKernelGGL(target_scan2d_kernel<PT_>, dim3(n_tiles), dim3(256), lds, ctx->stream, d_tab, e_steps, a_steps, ep.n_ants_x, ep.n_ants_y,         \
                       d_snap, n, part_val, part_idx);                                                                                                   \
  } while (0)
  if (pt == 64) ISAC_TARGET_SCAN2D(64); else if (pt == 32) ISAC_TARGET_SCAN2D(32); else ISAC_TARGET_SCAN2D(16);
#undef ISAC_TARGET_SCAN2D
  ISAC_HIP(hipGetLastError());
  hipLaunchKernelGGL(target_scan2d_reduce_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, (const double*)part_val, (const int*)part_idx, (int)n_tiles, n, d_bin);
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}

// scan bin -> degrees: music.m:103 (ULA), music.m:70-71 with j = e + eSteps a (UPA)
double azi_of_bin(int bin, const isac_est_params& ep) { return bin * ep.azimuth_scan_granularity - ep.azimuth_scan_scale / 2.0; }
double azi_of_bin2d(int j, int e_steps, const isac_est_params& ep) { return (j / e_steps) * ep.azimuth_scan_granularity - ep.azimuth_scan_scale / 2.0; }
double ele_of_bin2d(int j, int e_steps, const isac_est_params& ep) { return (j % e_steps) * ep.elevation_scan_granularity - ep.elevation_scan_scale / 2.0; }

}  // namespace

int target_scan_snapshots(isac_ctx* ctx, const c64* d_snap, int n, int* d_bin, double* azi, double* ele) {
  const Fft2dCpi& ts = ctx->tgt;
  const isac_est_params& ep = ts.ep;
  const int A = ts.A;
  int e_steps = 0;
  if (ep.array_is_upa) {
    const double* d_tab = nullptr;
    int a_steps = 0;
    ISAC_TRY(isac_doa2d_grid(ctx, &ep, A, &d_tab, &e_steps, &a_steps));
    ISAC_TRY(enqueue_scan2d(ctx, ep, A, d_tab, e_steps, a_steps, d_snap, n, d_bin));
  } else {
    const size_t lds = sizeof(c64) * (size_t)A;
    ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(target_azi_kernel), lds));
    hipLaunchKernelGGL(target_azi_kernel, dim3(n), dim3(256), lds, ctx->stream, d_snap, A, ts.d_sind, ts.n_steps, 0.5, d_bin);
    ISAC_HIP(hipGetLastError());
  }
  std::vector<int> bins((size_t)n);
  ISAC_TRY(copy_d2h(ctx, bins.data(), d_bin, sizeof(int) * (size_t)n));
  for (int i = 0; i < n; ++i) {
    azi[i] = ep.array_is_upa ? azi_of_bin2d(bins[(size_t)i], e_steps, ep) : azi_of_bin(bins[(size_t)i], ep);
    if (ep.array_is_upa) ele[i] = ele_of_bin2d(bins[(size_t)i], e_steps, ep);
  }
  return ISAC_OK;
}

int target_cells_of_planes(isac_ctx* ctx, const char* who, const PlaneCells& src, isac_target_list* out) { return select_cells(ctx, who, src, out, nullptr, 0, nullptr); }

extern "C" int isac_fft2d_get_targets(isac_ctx* ctx, isac_target_list* out, isac_c64* snapshots, int32_t cap_snap) {
  ISAC_ENTER(ctx);
  ISAC_TRY(cpi_ready(ctx, "isac_fft2d_get_targets", out, snapshots, cap_snap));
  const Fft2dCpi& ts = ctx->tgt;
  if (ts.ep.array_is_upa) return fail(ctx, ISAC_ERR_UNSUPPORTED, "isac_fft2d_get_targets: ULA only");
  const isac_est_params& ep = ts.ep;
  const int A = ts.A;
  SelectedCells sc;
  ISAC_TRY(select_cells(ctx, "isac_fft2d_get_targets", cpi_cells(ctx), out, snapshots, cap_snap, &sc));
  if (sc.n == 0) return ISAC_OK;
  const int n = sc.n;
  const c64* twd = nullptr;
  ISAC_TRY(isac_get_twiddles(ctx, ep.n_fft, &twd));
  const size_t lds = sizeof(c64) * (size_t)A;
  ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(target_doa_kernel), lds));
  hipLaunchKernelGGL(target_doa_kernel, dim3(n), dim3(256), lds, ctx->stream, (const c64*)ctx->ymid.p, ts.win.nr, ts.L, A, ep.n_fft, twd, std::sqrt((double)ep.n_fft),
                     (const int*)(sc.d + sc.off_sel), (const int*)(sc.d + sc.off_sel) + n, ts.d_sind, ts.n_steps, 0.5, (int*)(sc.d + sc.off_bin), (c64*)(sc.d + sc.off_snap));
  ISAC_HIP(hipGetLastError());
  std::vector<int> bins;
  ISAC_TRY(fetch_bins(ctx, sc, A, bins, snapshots));
  for (int i = 0; i < n; ++i) out->azi[i] = azi_of_bin(bins[(size_t)i], ep);
  out->n_targets = n;
  return ISAC_OK;
}

extern "C" int isac_fft2d_get_targets_upa(isac_ctx* ctx, isac_target_list* out, double* ele, isac_c64* snapshots, int32_t cap_snap) {
  ISAC_ENTER(ctx);
  if (!ele) return fail(ctx, ISAC_ERR_INVALID_ARG, "NULL argument");
  ISAC_TRY(cpi_ready(ctx, "isac_fft2d_get_targets_upa", out, snapshots, cap_snap));
  const Fft2dCpi& ts = ctx->tgt;
  if (!ts.ep.array_is_upa) return fail(ctx, ISAC_ERR_UNSUPPORTED, "isac_fft2d_get_targets_upa: a planar array only; isac_fft2d_get_targets is the list of a ULA");
  const isac_est_params& ep = ts.ep;
  const int A = ts.A;
  const double* d_tab = nullptr;
  int e_steps = 0, a_steps = 0;
  ISAC_TRY(isac_doa2d_grid(ctx, &ep, A, &d_tab, &e_steps, &a_steps));     // n_ants_x n_ants_y != A: ISAC_ERR_INVALID_ARG; A > 256: ISAC_ERR_UNSUPPORTED
  SelectedCells sc;
  ISAC_TRY(select_cells(ctx, "isac_fft2d_get_targets_upa", cpi_cells(ctx), out, snapshots, cap_snap, &sc));
  if (sc.n == 0) return ISAC_OK;
  const int n = sc.n;
  const c64* twd = nullptr;
  ISAC_TRY(isac_get_twiddles(ctx, ep.n_fft, &twd));
  c64* d_snap = (c64*)(sc.d + sc.off_snap);
  ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(target_snap_kernel), sizeof(c64) * (size_t)A));
  hipLaunchKernelGGL(target_snap_kernel, dim3(n), dim3(256), sizeof(c64) * (size_t)A, ctx->stream, (const c64*)ctx->ymid.p, ts.win.nr, ts.L, A, ep.n_fft, twd,
                     std::sqrt((double)ep.n_fft), (const int*)(sc.d + sc.off_sel), (const int*)(sc.d + sc.off_sel) + n, d_snap);
  ISAC_HIP(hipGetLastError());
  ISAC_TRY(enqueue_scan2d(ctx, ep, A, d_tab, e_steps, a_steps, d_snap, n, (int*)(sc.d + sc.off_bin)));
  std::vector<int> bins;
  ISAC_TRY(fetch_bins(ctx, sc, A, bins, snapshots));
  for (int i = 0; i < n; ++i) {
    out->azi[i] = azi_of_bin2d(bins[(size_t)i], e_steps, ep);
    ele[i] = ele_of_bin2d(bins[(size_t)i], e_steps, ep);
  }
  out->n_targets = n;
  return ISAC_OK;
}
