// Coefficient vectors of a multi-static echo (gfx950): path_coef_kernel and its host side, isac_path_coefs_on (include/isac_multistatic.h).
//
// A path p takes the waveform of source s_p [T x A_s], weights it with its transmit steering vector b_p, delays it by d_p samples, Doppler-shifts and scales it
// (basicRadarChannel.m:42-51 with b_p where the mono-static echo has a_q in e * a):
//   beam_p[u] = sum_a x_{s_p}[u, a] b_p[a]
//   coef_p[t] = g_p e^{j wd_p t Ts} e^{j w (t - d_p) Ts} beam_p[t - d_p] e^{-j w t Ts}      t >= d_p, else 0
// What echo.hip has for this stops short of it: beamsum_coef_kernel forms coef in one pass but for one source and two targets; beamsum_kernel + coef_kernel take any count but
// write a [P x T] beam array and read it back -- 2 P T 16 B that carry nothing -- and know one source.  path_coef_kernel sums with beam_sample and applies coef_value
// (echo_dev.hpp: the expressions of those kernels, so a mono-static path list gives their bits) and stores coef_p[u + d_p] from the thread that holds beam_p[u]: no beam array
// touches HBM.  Everything behind coef [P x T], phase_rx [T] and the receive steering vectors is echo.hip's (radar_waveform_kernel, demod_kernel, echo_spectral_kernel).
#include <algorithm>
#include <cstring>

#include "isac_internal.hpp"
#include "echo_dev.hpp"

namespace isac {

// The paths sorted by source and cut into tiles: up to kPathTile paths of ONE source, whose waveform the tile reads once.  A launch serves the tiles of one size QT.
struct PathDesc {
  TargetDesc td;            // wd = (2 pi) f_p, lsf = g_p, shift = min(d_p, T)
  long long steer_off;      // b_p starts here in the concatenated transmit steering vectors
  long long row;            // p: the row of coef this path writes
};
struct PathTile {
  const c64* tx;            // x_s [T x A]
  int A, first;             // its element count; the tile's paths are desc[first .. first + QT)
};

// Long-lived workgroups (grid-stride as in beamsum_kernel; one resident round of them, isac_path_coefs_on) walk the units (tile, block of 256 consecutive samples), tile by tile: the transmit steering vectors of
// the tile's paths sit in LDS [QT x A] while its blocks are walked.  Loads are 16 B per lane, unconditional, at a clamped sample; stores are conditional.  Every element of
// coef is written exactly once and by one thread: coef_p[t], t >= d_p, by the thread that summed sample t - d_p of p's tile, and the zero of coef_p[t], t < d_p, by the thread
// of sample t -- two paths with equal shifts write different rows, so nothing is accumulated and there are no atomics.  d_p >= T: the row is all zeros.
// phase_rx (not NULL in ONE launch of a call): its tile 0 also writes phase_rx[u] = rx_phase(w, u Ts), which rx_sample multiplies the noise with.
template <int QT, int UNROLL>
__global__ __launch_bounds__(256) void path_coef_kernel(const PathTile* __restrict__ tiles, int n_tiles, const PathDesc* __restrict__ desc, const c64* __restrict__ steer_tx,
                                                        long long T, double w /* (2*pi)*fc */, double Ts, c64* __restrict__ coef /* [P x T] */,
                                                        c64* __restrict__ phase_rx /* [T] or nullptr */) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  c64* s_steer = reinterpret_cast<c64*>(smem_raw);
  for (int i = 0; i < n_tiles; ++i) {                                    // (uniform: every workgroup walks every tile)
    const PathTile tl = tiles[i];
    const PathDesc* dq = desc + tl.first;
    if (i > 0) __syncthreads();                                          // the previous tile's last reads of s_steer
    for (int j = threadIdx.x; j < tl.A * QT; j += blockDim.x) {
      const int q = j / tl.A, a = j - q * tl.A;
      s_steer[j] = steer_tx[dq[q].steer_off + a];
    }
    __syncthreads();
    for (long long t0 = (long long)blockIdx.x * 256; t0 < T; t0 += (long long)gridDim.x * 256) {
      const long long u = t0 + threadIdx.x;
      const long long uc = u < T ? u : T - 1;                            // unconditional loads (clamped), conditional stores
      c64 acc[QT];
      beam_sample<QT, UNROLL>(tl.tx + uc, T, tl.A, s_steer, acc);
      if (u >= T) continue;                                              // (no barrier in this loop)
      if (phase_rx && i == 0) phase_rx[u] = rx_phase(w, (double)u * Ts);
#pragma unroll
      for (int q = 0; q < QT; ++q) {
        const TargetDesc td = dq[q].td;
        c64* cq = coef + dq[q].row * T;
        if (u < td.shift) cq[u] = mk(0.0, 0.0);
        const long long t = u + td.shift;                                // shift <= T: no overflow
        if (t < T) {
          const double tt = (double)t * Ts;
          cq[t] = coef_value(acc[q], t, td, w, Ts, tt, rx_phase(w, tt));
        }
      }
    }
  }
}

// The fractional delays of include/isac_subsample.h: D_p[k, l] <- D_p[k, l] exp(-2 pi j (c_p + (k - n_sc/2) delta_p / Nfft)), c_p = frac(fc delta_p / fs) formed on the
// host.  One thread per element of a path's grid (blockIdx.y = p), k fastest; the turn count is reduced modulo 1 before one sincospi.  delta_p == 0: the path's workgroups
// return at once (uniform) and its values keep their bits.
struct PathFracArg { double carrier[ISAC_MULTISTATIC_MAX_PATHS], delta[ISAC_MULTISTATIC_MAX_PATHS]; };
__global__ __launch_bounds__(256) void path_frac_ramp_kernel(c64* __restrict__ D /* [n_sc x L_whole x P] */, int n_sc, long long per_path /* n_sc L_whole */, double nfft, PathFracArg f) {
  const int p = blockIdx.y;
  const double delta = f.delta[p];
  if (delta == 0.0) return;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= per_path) return;
  const int k = (int)(i % n_sc);
  double t = f.carrier[p] + ((double)(k - n_sc / 2) * delta) / nfft;     // turns
  t -= rint(t);
  double s, co;
  sincospi(-2.0 * t, &s, &co);
  c64* d = D + per_path * p + i;
  *d = *d * mk(co, s);
}

}  // namespace isac

using namespace isac;

int isac_path_frac_ramp_on(isac_ctx* ctx, hipStream_t st, const PathFrac& f, int n_sc, int nfft, int L_whole, int n_paths) {
  PathFracArg arg{};
  for (int p = 0; p < n_paths; ++p) {
    const double turns = f.fc * f.frac[p] / f.fs;
    arg.carrier[p] = turns - std::floor(turns);
    arg.delta[p] = f.frac[p];
  }
  const long long per_path = (long long)n_sc * L_whole;
  hipLaunchKernelGGL(path_frac_ramp_kernel, dim3(cdiv(per_path, 256), (unsigned)n_paths), dim3(256), 0, st, (c64*)ctx->dgrid.p, n_sc, per_path, (double)nfft, arg);
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}

constexpr int kPathTile = 8;

int isac_path_coefs_on(isac_ctx* ctx, hipStream_t st, const PathCoefJob& j) {
  const int P = j.n_paths, A = j.n_ants;
  const long long T = j.T;
  // paths by source (stable: input order inside a source), tiles of min(rest, 8) paths, tiles by size
  std::vector<int> order(P);
  for (int p = 0; p < P; ++p) order[p] = p;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return j.path_source[a] < j.path_source[b]; });
  std::vector<long long> steer_off(P);
  long long n_tx_steer = 0;
  for (int p = 0; p < P; ++p) { steer_off[p] = n_tx_steer; n_tx_steer += j.n_ants_src[j.path_source[p]]; }
  const double two_pi = 2.0 * M_PI;
  std::vector<PathDesc> desc(P);
  for (int i = 0; i < P; ++i) {
    const int p = order[i];
    desc[i].td.wd = two_pi * j.path_doppler_hz[p];                       // 2j*pi*fd  basicRadarChannel.m:44
    desc[i].td.lsf = j.path_gain[p];                                     // :48
    desc[i].td.shift = std::min<long long>(j.path_shift[p], T);          // :22; a path at or beyond T contributes nothing
    desc[i].steer_off = steer_off[p];
    desc[i].row = p;
  }
  std::vector<PathTile> by_size[kPathTile + 1];
  for (int i = 0; i < P;) {
    const int s = j.path_source[order[i]];
    int n = 1;
    while (i + n < P && n < kPathTile && j.path_source[order[i + n]] == s) ++n;
    by_size[n].push_back(PathTile{j.d_tx[s], j.n_ants_src[s], i});
    i += n;
  }
  // receive steering: [A x P] and its transpose (row r holds a_p[r] at r P + p), the layout of ctx->steer the synthesis kernels read
  std::vector<c64> rx(2 * (size_t)A * P);
  for (int p = 0; p < P; ++p)
    for (int a = 0; a < A; ++a) {
      const isac_c64 v = j.path_rx_steering[(size_t)a + (size_t)A * p];
      rx[(size_t)p * A + a] = rx[(size_t)A * P + (size_t)a * P + p] = mk(v.re, v.im);
    }
  MetaPack pack;
  pack.add(rx);
  const size_t off_tx = pack.add(j.path_tx_steering, sizeof(c64) * (size_t)n_tx_steer);
  const size_t off_desc = pack.add(desc);
  size_t off_tiles[kPathTile + 1] = {};
  for (int n = 1; n <= kPathTile; ++n) off_tiles[n] = pack.add(by_size[n]);
  ISAC_TRY(ensure(ctx, ctx->coef, sizeof(c64) * (size_t)P * T));
  ISAC_TRY(ensure(ctx, ctx->phase_rx, sizeof(c64) * (size_t)T));
  ISAC_TRY(pack.upload(ctx, ctx->steer));                                // (staged on ctx->stream: st is that stream, or ordered behind it)
  const char* base = (const char*)ctx->steer.p;
  int n_cus = 0;
  ISAC_TRY(ctx_n_cus(ctx, &n_cus));
  const double w = two_pi * j.fc, Ts = 1.0 / j.fs;                       // basicRadarChannel.m:30,73; :15
  c64* prx = (c64*)ctx->phase_rx.p;
  auto launch = [&](auto qc) {
    constexpr int QT = decltype(qc)::value;
    const std::vector<PathTile>& tl = by_size[QT];
    if (tl.empty()) return;
    int a_max = 0;
    for (const PathTile& t : tl) a_max = std::max(a_max, t.A);
    auto kern = path_coef_kernel<QT, (QT <= 2 ? 32 : 8)>;                 // the antenna unroll of beamsum_kernel at this QT
    const size_t lds = sizeof(c64) * (size_t)a_max * QT;
    // One round of workgroups: with coef_value in the same wave the kernel holds 123-138 VGPRs, three waves per SIMD, so of the beam-sum's 1024 workgroups 768 are
    // resident and the last 256 run alone behind them (measured at the bench shape: 234 us against 179 us of beamsum_kernel + coef_kernel); the grid is what is resident.
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, 256, lds) != hipSuccess || per_cu < 1) per_cu = 1;
    const unsigned grid = (unsigned)std::min<long long>(cdiv(T, 256), (long long)per_cu * n_cus);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, st,
                       (const PathTile*)(base + off_tiles[QT]), (int)tl.size(), (const PathDesc*)(base + off_desc), (const c64*)(base + off_tx), T, w, Ts, (c64*)ctx->coef.p, prx);
    prx = nullptr;                                                       // the first launch has written phase_rx
  };
  launch(std::integral_constant<int, 8>{}); launch(std::integral_constant<int, 7>{}); launch(std::integral_constant<int, 6>{}); launch(std::integral_constant<int, 5>{});
  launch(std::integral_constant<int, 4>{}); launch(std::integral_constant<int, 3>{}); launch(std::integral_constant<int, 2>{}); launch(std::integral_constant<int, 1>{});
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}
