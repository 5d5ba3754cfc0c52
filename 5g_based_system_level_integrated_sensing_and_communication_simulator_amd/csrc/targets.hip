// Per-target list of fft2D (gfx950 only): isac_fft2d_get_targets joins what the last completed fft2D left on the context -- the range rows ymid [rows x L x A], the power
// window pwin [nr x nc x A] and the per-antenna CFAR lists -- into paired (range, velocity, azimuth) entries.  Project-defined (include/isac_targets.h):
//   1  S = sum over antennas of the power window (fp64, ascending antenna order from 0.0); hits = antennas whose CFAR list holds the cell
//   2  target cell = CUT cell with hits >= 1 and S strictly above all 8 neighbours
//   3  snapshot x[a] = rdm(r, c, a): a single-bin DFT over the L symbols of row r (the expression of doppler_pow_kernel before the modulus)
//   4  azimuth = first arg-max of the Bartlett scan |a_i' x|^2 over MUSIC's ULA grid (same sind table, same steering expression as music_scan_kernel)
//   5  host: sort by S descending, ties by ascending column-major index; rng / vel as fft2D.m:77-82
// K1 target_hits_kernel scatters the lists into a zeroed hits map (its own launch: the map must be complete before any cell is tested), K2 target_cells_kernel sums, tests and
// compacts, K3 target_doa_kernel forms snapshot and azimuth of every selected cell.  All three are latency-bound (a few MB at the bench shape) and off the timed path.
#include <algorithm>
#include <numeric>

#include "isac_internal.hpp"

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

__global__ __launch_bounds__(kCellR * kCellC) void target_cells_kernel(const double* __restrict__ pwin /* [nr x nc x A] */, int nr, int nc, int A, int hr, int hc,
                                                                       int n_cut_rows, int n_cut_cols, const int* __restrict__ hits,
                                                                       unsigned* __restrict__ count, int* __restrict__ cand_cut /* [n_cut] CUT ordinal */,
                                                                       int* __restrict__ cand_hits, double* __restrict__ cand_s) {
  constexpr int SR = kCellR + 2, SC = kCellC + 2;
  __shared__ double s_s[SC * SR];                                         // column-major tile + rim
  const int tid = threadIdx.x;
  const int r0 = blockIdx.x * kCellR, c0 = blockIdx.y * kCellC;           // first CUT row / column of the tile (0-based)
  const long long plane = (long long)nr * nc;
  for (int i = tid; i < SR * SC; i += kCellR * kCellC) {
    const int lr = i % SR, lc = i / SR;
    const int wr = hr + r0 + lr - 1, wc = hc + c0 + lc - 1;               // window coordinates (hr, hc >= 1: never negative)
    double s = __builtin_nan("");                                          // past the window (a tile that overhangs the zone): never a valid cell's neighbour
    if (wr < nr && wc < nc) {
      const double* p = pwin + wr + (long long)nr * wc;
      s = 0.0;
      for (int a = 0; a < A; ++a) s = __dadd_rn(s, p[plane * a]);         // ascending antenna order, from 0.0
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
    }
  }
}

// ---------------------------------------------------------------- K3: array snapshot + Bartlett azimuth of one target cell per workgroup
// Phase 1: x[a] = rdm(r, c, a) in LDS.  Four lanes share an antenna, each runs doppler_pow_kernel's multiply-add chain over a quarter of the symbols; the quarters are
// added pairwise ((q0 + q1) + (q2 + q3): fp addition commutes, so all four lanes hold the same bits).
// Phase 2: one lane per scan angle reads x[m] from LDS -- every lane the same address, a broadcast: no bank conflict whatever the c64 layout -- and forms
// B = |sum_m conj(a[m]) x[m]|^2; angles with bitwise equal sind (mirror twins) run the same instructions on the same operands.  Arg-max: each lane keeps its first
// maximum in ascending angle order, then a fixed tree on (value, lowest index).
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
  const int row = cell_row[t], c = cell_col[t];
  const int Lu = L < n_fft ? L : n_fft;                                   // fft(., nFFT, 2) truncates when L > nFFT
  const int half = L / 2;                                                 // ifftshift over the symbols
  const int kbin = (c + n_fft / 2) % n_fft;                               // fftshift: column c <-> bin (c + nFFT/2) mod nFFT
  const int chunk = (Lu + 3) / 4;
  for (int base = 0; base < 4 * A; base += 256) {                         // (256 = 64 quads: a quad is inside one wave and all of it active or none)
    const int a = (base + tid) >> 2, part = tid & 3;
    c64 acc = mk(0.0, 0.0);
    if (a < A) {
      const int li0 = part * chunk, li1 = min(li0 + chunk, Lu);
      int m = (int)(((long long)li0 * kbin) % n_fft);
      const c64* col = ymid + row + (long long)n_rows * L * a;
      for (int li = li0; li < li1; ++li) {
        int lsrc = li + half;
        if (lsrc >= L) lsrc -= L;
        acc = fma(col[(long long)n_rows * lsrc], tw_d[m], acc);
        m += kbin;
        if (m >= n_fft) m -= n_fft;
      }
    }
    acc.re += __shfl_xor(acc.re, 1); acc.im += __shfl_xor(acc.im, 1);
    acc.re += __shfl_xor(acc.re, 2); acc.im += __shfl_xor(acc.im, 2);
    if (a < A && part == 0) s_x[a] = mk(acc.re / sqrt_nfft, acc.im / sqrt_nfft);   // fft(.)/sqrt(nFFT)  fft2D.m:46
  }
  __syncthreads();
  for (int a = tid; a < A; a += 256) snap[a + (long long)A * t] = s_x[a];
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
  if (tid == 0) azi_bin[t] = s_idx[0] == 0x7fffffff ? 0 : s_idx[0];
}

}  // namespace isac

// ================================================================= host side
using namespace isac;

extern "C" int isac_fft2d_get_targets(isac_ctx* ctx, isac_target_list* out, isac_c64* snapshots, int32_t cap_snap) {
  ISAC_ENTER(ctx);
  if (!out || (snapshots && cap_snap < 0)) return fail(ctx, ISAC_ERR_INVALID_ARG, "NULL argument");
  const Fft2dCpi& ts = ctx->tgt;
  if (!ctx->last.valid || ts.state != Fft2dCpi::kCollected)
    return fail(ctx, ISAC_ERR_INVALID_ARG, "isac_fft2d_get_targets: no completed fft2D on this context whose range rows, power window and detection lists are still on the device");
  if (ts.ep.array_is_upa) return fail(ctx, ISAC_ERR_UNSUPPORTED, "isac_fft2d_get_targets: ULA only");
  const isac_est_params& ep = ts.ep;
  const CutWindow& w = ts.win;
  const int hr = w.hr, hc = w.hc;
  if (hr < 1 || hc < 1) return fail(ctx, ISAC_ERR_UNSUPPORTED, "isac_fft2d_get_targets: the local-maximum test needs a halo of at least one cell (guard + training) in both dimensions");
  const int A = ts.A, L = ts.L, nr = w.nr, nc = w.nc, n_cut_rows = w.n_cut_rows, n_cut_cols = w.n_cut_cols, n_cut = (int)w.n_cut();
  std::memset(out, 0, sizeof(*out));
  // one scratch block: [hits nr x nc | count (16 ints)] zeroed, then the candidate lists, the selected cells and their results
  const size_t n_map = (size_t)nr * nc;
  const size_t off_cnt = sizeof(int) * n_map, off_ccut = off_cnt + 64, off_chit = off_ccut + sizeof(int) * (size_t)n_cut;
  const size_t off_cs = (off_chit + sizeof(int) * (size_t)n_cut + 15) & ~(size_t)15, off_sel = off_cs + sizeof(double) * (size_t)n_cut;
  const size_t off_azi = off_sel + sizeof(int) * 2 * ISAC_MAX_TARGETS, off_snap = (off_azi + sizeof(int) * ISAC_MAX_TARGETS + 15) & ~(size_t)15;
  ISAC_TRY(ensure(ctx, ctx->tgt_scratch, off_snap + sizeof(c64) * (size_t)A * ISAC_MAX_TARGETS));
  char* d = (char*)ctx->tgt_scratch.p;
  const c64* twd = nullptr;
  ISAC_TRY(isac_get_twiddles(ctx, ep.n_fft, &twd));
  ISAC_HIP(hipMemsetAsync(d, 0, off_ccut, ctx->stream));
  hipLaunchKernelGGL(target_hits_kernel, dim3(std::min(cdiv(ts.cap, 256), 8u), A), dim3(256), 0, ctx->stream, (const int*)ctx->det_cut.p, (const int*)ctx->det_cnt.p, ts.cap,
                     n_cut_rows, n_cut, hr, hc, nr, (int*)d);
  ISAC_HIP(hipGetLastError());
  hipLaunchKernelGGL(target_cells_kernel, dim3(cdiv(n_cut_rows, kCellR), cdiv(n_cut_cols, kCellC)), dim3(kCellR * kCellC), 0, ctx->stream, (const double*)ctx->pwin.p, nr, nc,
                     A, hr, hc, n_cut_rows, n_cut_cols, (const int*)d, (unsigned*)(d + off_cnt), (int*)(d + off_ccut), (int*)(d + off_chit), (double*)(d + off_cs));
  ISAC_HIP(hipGetLastError());
  unsigned count = 0;
  ISAC_TRY(copy_d2h(ctx, &count, d + off_cnt, sizeof(count)));
  if (count > (unsigned)n_cut) return fail(ctx, ISAC_ERR_HIP, "internal: more target cells than CUTs");
  const int n_total = (int)count;
  out->n_total = n_total;
  if (n_total == 0) return ISAC_OK;
  std::vector<int> ccut((size_t)n_total), chit((size_t)n_total);
  std::vector<double> cs((size_t)n_total);
  ISAC_TRY(copy_d2h(ctx, ccut.data(), d + off_ccut, sizeof(int) * (size_t)n_total));
  ISAC_TRY(copy_d2h(ctx, chit.data(), d + off_chit, sizeof(int) * (size_t)n_total));
  ISAC_TRY(copy_d2h(ctx, cs.data(), d + off_cs, sizeof(double) * (size_t)n_total));
  // S descending, ties by ascending column-major index r + nIFFT (c - 1) -- the order of the CUT ordinal cr + n_cut_rows cc (column first, then row)
  std::vector<int> order((size_t)n_total);
  std::iota(order.begin(), order.end(), 0);
  std::sort(order.begin(), order.end(), [&](int p, int q) {
    if (cs[(size_t)p] != cs[(size_t)q]) return cs[(size_t)p] > cs[(size_t)q];
    return ccut[(size_t)p] < ccut[(size_t)q];
  });
  const int n = std::min(n_total, (int)ISAC_MAX_TARGETS);
  if (snapshots && n > cap_snap) return fail(ctx, ISAC_ERR_CAPACITY, "isac_fft2d_get_targets: more targets than snapshot columns");
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
    sel[(size_t)i] = rc.row - w.first_row;
    sel[(size_t)n + i] = rc.col - 1;
  }
  ISAC_TRY(stage_upload(ctx, d + off_sel, sel.data(), sizeof(int) * sel.size()));
  const size_t lds = sizeof(c64) * (size_t)A;
  ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(target_doa_kernel), lds));
  hipLaunchKernelGGL(target_doa_kernel, dim3(n), dim3(256), lds, ctx->stream, (const c64*)ctx->ymid.p, nr, L, A, ep.n_fft, twd, std::sqrt((double)ep.n_fft),
                     (const int*)(d + off_sel), (const int*)(d + off_sel) + n, ts.d_sind, ts.n_steps, 0.5, (int*)(d + off_azi), (c64*)(d + off_snap));
  ISAC_HIP(hipGetLastError());
  std::vector<int> bins((size_t)n);
  ISAC_TRY(copy_d2h(ctx, bins.data(), d + off_azi, sizeof(int) * (size_t)n));
  if (snapshots) ISAC_TRY(copy_d2h(ctx, snapshots, d + off_snap, sizeof(c64) * (size_t)A * n));
  for (int i = 0; i < n; ++i) out->azi[i] = bins[(size_t)i] * ep.azimuth_scan_granularity - ep.azimuth_scan_scale / 2.0;   // music.m:103
  out->n_targets = n;
  return ISAC_OK;
}
