// Echo synthesis + CP-OFDM (de)modulation kernels (gfx950).
//
// Reference path: sensing.monoStaticSensing (+sensing/monoStaticSensing.m:1-23) ->
// sensing.channelModels.basicRadarChannel (+sensing/+channelModels/basicRadarChannel.m:1-76)
// -> nrOFDMDemodulate.  The reference makes ~10 full passes over the [T x A] waveform;
// here the rank-1 structure of basicRadarChannel.m:51  (e * a) * a.'  is used to read the
// transmit waveform ONCE (beam-sum), build one length-T coefficient vector per LoS target,
// and synthesise each receive antenna's samples directly inside the OFDM-demodulation
// FFT's register file, so rxWaveform never touches HBM:
//
//   beam_q[t]   = sum_a tx[t,a] * a_q[a]                                   (1 read of tx)
//   coef_q[t]   = lsf_q * e^{j wd_q t} * e^{j w (t-d_q)} * beam_q[t-d_q] * e^{-j w t}
//   rx[t,r]     = sum_q coef_q[t] * a_q[r] + sqrt(N0/2) * noise[t,r] * e^{-j w t}
//   echoGrid    = OFDM-demodulate(rx)                                      (1 write of grid)
//
// Carrier phase arguments are formed exactly like the reference forms them
// ((2*pi*fc) * (n*Ts), all in fp64) so the ~1e-8 rad rounding of those huge arguments
// is reproduced rather than "improved".
#include <cstring>
#include <type_traits>

#include "isac_internal.hpp"
#include "fft_lds.hpp"
#include "echo_dev.hpp"
#include "../../include/isac_subsample.h"
#include "beam_window.hpp"

namespace isac {

// ---------------------------------------------------------------- beam-sum: 1 read of tx
// HBM-bound: T x A x 16 B read once (1.007 GB at the bench shape), nothing else.  Each workgroup walks blocks of 256 consecutive samples
// (grid-stride: 1024 long-lived workgroups, four per CU) with its antenna loop unrolled UNROLL deep: 170.6 us = 5.90 TB/s, against 178 us of the
// 8-deep one-block-per-workgroup form of rounds 1-3 (profiles/r04_beamsum_sweep.txt; a plain streaming read tops out at 6.0-6.2 TB/s, tools/gbench.hip).
// One sample's sums over the antennas: beam_sample (echo_dev.hpp).
template <int QT, int UNROLL>
__global__ __launch_bounds__(256) void beamsum_kernel(const c64* __restrict__ tx, long long T, int A,
                                                      const c64* __restrict__ steer /* [A x QT] compacted LoS */,
                                                      c64* __restrict__ beam /* [QT x T] */) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  c64* s_steer = reinterpret_cast<c64*>(smem_raw);
  for (int i = threadIdx.x; i < A * QT; i += blockDim.x) s_steer[i] = steer[i];
  __syncthreads();
  for (long long t0 = (long long)blockIdx.x * 256; t0 < T; t0 += (long long)gridDim.x * 256) {
    const long long t = t0 + threadIdx.x;
    const long long tc = t < T ? t : T - 1;                            // unconditional loads (clamped), one conditional store
    c64 acc[QT];
    beam_sample<QT, UNROLL>(tx + tc, T, A, s_steer, acc);
    if (t < T) {
#pragma unroll
      for (int q = 0; q < QT; ++q) beam[(long long)q * T + t] = acc[q];
    }
  }
}

// ---------------------------------------------------------------- per-target coefficient vectors (TargetDesc, rx_phase, coef_value: echo_dev.hpp)
struct TargetTable {
  TargetDesc t[kMaxTargets];
};

__global__ __launch_bounds__(256) void coef_kernel(const c64* __restrict__ beam, long long T, int Q,
                                                   TargetTable tab, double w /* (2*pi)*fc */, double Ts,
                                                   c64* __restrict__ coef /* [Q x T] */,
                                                   c64* __restrict__ phase_rx /* [T] */) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= T) return;
  double tt = (double)t * Ts;
  c64 prx = rx_phase(w, tt);
  phase_rx[t] = prx;
  for (int q = 0; q < Q; ++q) {
    long long d = tab.t[q].shift;
    c64 out = mk(0.0, 0.0);
    if (t >= d) out = coef_value(beam[(long long)q * T + (t - d)], t, tab.t[q], w, Ts, tt, prx);
    coef[(long long)q * T + t] = out;
  }
}

// The beam-sum that writes the coefficient vectors itself (the spectral route of isac_mono_static_sensing_fused_dev, one or two LoS targets): that route reads neither beam
// nor phase_rx, and coef_kernel was a launch of its own on the serial chain of the CPI -- 12-13 us plus its gap, for ~300 VALU instructions per sample that fit in the shadow
// of this kernel's loads.  The thread that has summed sample u of target q holds beam_q[u] = the only input of coef_q[u + d_q] (coef_value above: the bits of coef_kernel);
// a sample before the waveform (u < 0, beam_window.hpp) stands for the zero of coef_q[u + d_q]; samples with u + d_q >= T are dropped.
//
// It sums only the samples the demodulation windows need (beam_window.hpp: nfft + d_max - d_min per symbol, nothing of the cyclic prefix in between -- 6.6 % of the 1 GB at
// the bench shape), so the elements of coef OUTSIDE every window stay unwritten: every element some window reads is written exactly once.  The workgroups are long-lived as
// in beamsum_kernel, walking units (symbol, 256 samples of its range) instead of blocks of [0, T); a wave whose 64 samples lie outside its symbol's share loads nothing.
// Measured (profiles/r08_ab_parent_vs_pr.txt): alone on the GPU the kernel takes what the walk over [0, T) took, 177-180 us -- the bytes saved buy no isolated time; with other
// CPIs' kernels beside it the pipelined rate gains 0.8-1.3 % from the walk and 1.1-1.9 % more from the upload that is gone (below).
//
// The steering vectors come in the argument block where they fit (steer == nullptr: A QT <= kSteerArgMax; read by address from the constant argument segment, never copied
// to private memory), which takes the staged upload -- a blit kernel of 4-6 us at the head of every CPI's serial chain -- off this route; workgroup 0 then writes both halves
// of ctx->steer ([QT x A] and its transpose) for the kernels behind it in the stream.
template <int QT>
struct CoefTargets {
  TargetDesc t[QT];
};
template <int QT, int UNROLL>
__global__ __launch_bounds__(256) void beamsum_coef_kernel(const c64* __restrict__ tx, long long T, int A,
                                                           const c64* __restrict__ steer /* [A x QT] compacted LoS, or nullptr: steer_arg */,
                                                           const SteerArg steer_arg, c64* __restrict__ steer_out /* [2 x A x QT], written when steer == nullptr */,
                                                           BeamWindow bw, CoefTargets<QT> tab, double w /* (2*pi)*fc */, double Ts,
                                                           c64* __restrict__ coef /* [QT x T] */) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  c64* s_steer = reinterpret_cast<c64*>(smem_raw);
  if (steer) {
    for (int i = threadIdx.x; i < A * QT; i += blockDim.x) s_steer[i] = steer[i];
  } else {
    for (int i = threadIdx.x; i < A * QT; i += blockDim.x) {
      const c64 v = steer_arg.v[i];
      s_steer[i] = v;
      if (blockIdx.x == 0) {
        const int q = i / A, a = i - q * A;
        steer_out[i] = v;
        steer_out[A * QT + a * QT + q] = v;          // row r of the transpose holds a_q[r] at r QT + q
      }
    }
  }
  __syncthreads();
  const int n_units = (int)bw_units(bw);
  for (int k = blockIdx.x; k < n_units; k += gridDim.x) {
    const int l = k / bw.units_per_symbol, j = k - l * bw.units_per_symbol;
    const long long lo = bw_first(bw, l), hi = bw_range_end(bw, l);
    const long long u = bw_sample(bw, l, j, threadIdx.x);
    const bool mine = u >= lo && u < hi;
    if (!__any(mine)) continue;                                        // (wave-uniform; no barrier in this loop)
    long long uc = u < lo ? lo : u < hi ? u : hi - 1;                  // unconditional loads, clamped into the symbol's share (no line beyond it) and into [0, T);
    uc = uc < 0 ? 0 : uc < T ? uc : T - 1;                             // conditional stores
    c64 acc[QT];
    beam_sample<QT, UNROLL>(tx + uc, T, A, s_steer, acc);
    if (!mine) continue;
#pragma unroll
    for (int q = 0; q < QT; ++q) {
      const long long t = u + tab.t[q].shift;
      c64* cq = coef + (long long)q * T;
      if (t >= 0 && t < T) {
        const double tt = (double)t * Ts;
        cq[t] = u < 0 ? mk(0.0, 0.0) : coef_value(acc[q], t, tab.t[q], w, Ts, tt, rx_phase(w, tt));
      }
    }
  }
}

// The coefficient vectors inside the demodulation windows from beam-sums that are already in memory (the split lazy covariance: cov_noise_beam_kernel, cov.hip, sums the
// same BeamWindow units beside its MFMA stream and stores beam_q[u]): beamsum_coef_kernel's own tail, one workgroup per unit -- the same expression on the same bits, and like
// it nothing outside the windows is read or written (coef_kernel would walk [0, T) and read the beam-sum's holes).
template <int QT>
__global__ __launch_bounds__(256) void coef_window_kernel(const c64* __restrict__ beam /* [QT x T] */, long long T, BeamWindow bw, CoefTargets<QT> tab, double w, double Ts,
                                                          c64* __restrict__ coef /* [QT x T] */) {
  const int k = blockIdx.x;
  const int l = k / bw.units_per_symbol, j = k - l * bw.units_per_symbol;
  const long long lo = bw_first(bw, l), hi = bw_range_end(bw, l);
  const long long u = bw_sample(bw, l, j, threadIdx.x);
  if (!(u >= lo && u < hi)) return;
#pragma unroll
  for (int q = 0; q < QT; ++q) {
    const long long t = u + tab.t[q].shift;
    if (t >= 0 && t < T) {
      const double tt = (double)t * Ts;
      coef[(long long)q * T + t] = u < 0 ? mk(0.0, 0.0) : coef_value(beam[(long long)q * T + u], t, tab.t[q], w, Ts, tt, rx_phase(w, tt));
    }
  }
}

__global__ __launch_bounds__(256) void radar_waveform_kernel(long long T, int A, int Q, const c64* __restrict__ coef,
                                                             const c64* __restrict__ steer_rq /* [A x Q] row r: a_q[r] at r*Q+q */,
                                                             const c64* __restrict__ phase_rx, int noise_mode,
                                                             const c64* __restrict__ noise, double n0s, uint64_t seed,
                                                             c64* __restrict__ rx) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  int r = blockIdx.y;
  if (t >= T) return;
  rx[t + T * r] = rx_sample(t, r, T, Q, coef, steer_rq + (long long)r * Q, phase_rx, noise_mode, noise, n0s, seed);
}

// ---------------------------------------------------------------- fused sample synthesis + OFDM demodulation
struct OfdmGeom {
  int nfft, n_sc, cp_base, cp_long, sym_per_half;
};

// QT > 0: the number of LoS targets as a compile-time constant (a run-time target loop inside the 16 unrolled sample
// producers sends the register allocator to 256 VGPRs + scratch); QT = 0: any count.
template <class FFT, bool SYNTH, int QT = 0>
__global__ __launch_bounds__(256, 2) void demod_kernel(OfdmGeom g, long long T, int A, int L_whole, int L_out,
                                                       const c64* __restrict__ tw,
                                                       // SYNTH = true: synthesise rx samples
                                                       int Q_rt, const c64* __restrict__ coef,
                                                       const c64* __restrict__ steer_rq, const c64* __restrict__ phase_rx,
                                                       int noise_mode, const c64* __restrict__ noise, double n0s,
                                                       uint64_t seed,
                                                       // SYNTH = false: read them
                                                       const c64* __restrict__ wave,
                                                       c64* __restrict__ grid, const c64* __restrict__ logtab_g,
                                                       // SYNTH = false, optional: zero_flag[column] = 1 where every value stored for the column is +-0, else 0
                                                       // (NaN counts as non-zero) -- the D half of echo_range_xc_kernel's dead-column test
                                                       int* __restrict__ zero_flag) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  c64* lds = reinterpret_cast<c64*>(smem_raw);
  const int tid = threadIdx.x;
  FFT fft;
  bool stored_nz = false;
  constexpr bool kTables = SYNTH && QT > 0 && std::is_same<FFT, Fft4096>::value;   // LDS tables for the Philox Box-Muller
  const int Q = QT ? QT : Q_rt;
  {
    // one (symbol, antenna) column per workgroup, symbol fastest: consecutive workgroups write consecutive
    // 52 KB columns of one antenna plane.  (Antenna-fastest order would re-use a symbol's coef window in L2
    // -- rocprof shows 1.4 GB of coef/phase re-fetch from the Infinity Cache here -- but it scatters the
    // grid writes over 64 planes 11.7 MB apart and measured 15-20 % slower.)
    const int col = blockIdx.x;
    const int l = col % L_whole, r = col / L_whole;
    const int cp = cp_of_symbol(l, g.cp_base, g.cp_long, g.sym_per_half);
    const int off = cp / 2;  // fix(cp * CyclicPrefixFraction), fraction 0.5
    const long long w0 = symbol_start(l, g.nfft, g.cp_base, g.cp_long, g.sym_per_half) + off;
    const int dshift = cp - off;  // window leads the useful part by dshift samples
    if constexpr (SYNTH) {
      const c64* sr = steer_rq + (long long)r * Q;
      if (noise_mode == ISAC_NOISE_PHILOX) {
        // Box-Muller per sample is register hungry: interleave at most 4 producers.  At Nfft = 4096 the transform's own
        // W256 table (angle) and a 2 KB log table (radius) in LDS replace libm's sincospi / log (tools/dbench.hip:
        // 272 -> 222 us of VALU time per launch), so the tables go in first.
        if constexpr (kTables) {
          c64* lt = lds + FFT::LDS_ELEMS;
          if (tid < kLogTabSize) lt[tid] = logtab_g[tid];
          fft.init_table(lds, tw, tid);
          const c64* w256 = lds + FFT::IMG;
          fft.template fill<4>([&](int n) { return rx_sample(w0 + n, r, T, Q, coef, sr, phase_rx, ISAC_NOISE_PHILOX, noise, n0s, seed, w256, lt); }, tid);
          fft.init_twiddles(tw, tid);
        } else {
          fft.template fill<4>([&](int n) { return rx_sample(w0 + n, r, T, Q, coef, sr, phase_rx, ISAC_NOISE_PHILOX, noise, n0s, seed); }, tid);
        }
      } else {
        const int nm = (noise_mode == ISAC_NOISE_INJECTED) ? ISAC_NOISE_INJECTED : ISAC_NOISE_NONE;   // no generator code on this path
        fft.template fill<8>([&](int n) { return rx_sample(w0 + n, r, T, Q, coef, sr, phase_rx, nm, noise, n0s, seed); }, tid);
      }
    } else {
      const c64* src = wave + w0 + T * (long long)r;
      fft.fill([&](int n) { return src[n]; }, tid);
    }
    // after the fill: the twiddle-table loads fly together with the column's loads
    if (!(kTables && noise_mode == ISAC_NOISE_PHILOX)) fft.init(lds, tw, tid);
    fft.template transform<-1>(lds, tw, tid);
    c64* dst = grid + (long long)g.n_sc * ((long long)l + (long long)L_out * r);
    const int half = g.n_sc / 2;
    fft.drain(
        [&](int k, c64 v) {
          const int kb = (k < g.nfft / 2) ? k : k - g.nfft;  // signed bin
          const int row = kb + half;
          const c64 ph = fft.phase_ramp(lds, tw, kb, dshift);   // exp(+2 pi j kb dshift / nfft), fetched unconditionally
          if (row >= 0 && row < g.n_sc) {
            // streaming store: the 0.75 GB grid is not re-read by this kernel, keep L2 for the coef / phase vectors
            // that all 64 antennas share (tools/dbench.hip: 495 -> 463 us)
            const c64 o = v * ph;
            __builtin_nontemporal_store(o.re, &dst[row].re);
            __builtin_nontemporal_store(o.im, &dst[row].im);
            if constexpr (!SYNTH) stored_nz |= (o.re != 0.0) | (o.im != 0.0);
          }
        },
        tid);
    if constexpr (!SYNTH) {
      if (zero_flag) {                                                   // (uniform)
        const int any = __syncthreads_or(stored_nz);
        if (tid == 0) zero_flag[col] = any ? 0 : 1;
      }
    }
  }
}

// ---------------------------------------------------------------- spectral echo synthesis (performance noise modes)
// By linearity of the OFDM demodulator the echo grid of basicRadarChannel.m:64-74 + nrOFDMDemodulate is
//     echoGrid[k,l,r] = sum_q a_q[r] * D_q[k,l] + W[k,l,r],   D_q = OFDM-demodulate(coef_q)   (Q columns per symbol, not A)
// with W the demodulated AWGN -- i.i.d. CN(0, 2 Nfft s^2) on the kept bins (echo_dev.hpp).  With the noise drawn there
// (ISAC_NOISE_PHILOX_SPECTRAL) or supplied there (ISAC_NOISE_INJECTED_SPECTRAL) the A x L demodulation FFTs shrink to
// Q x L and the synthesis becomes a streaming rank-Q update: one write of the grid, VALU work = the generator only.
// One (symbol, antenna) column per workgroup, symbol fastest (as in demod_kernel).
template <int QT, int NZ>
__global__ __launch_bounds__(256) void echo_spectral_kernel(int K, int L_whole, int L_out, int A, int Q_rt, const c64* __restrict__ D,
                                                            const c64* __restrict__ steer_rq, double sig, uint64_t seed,
                                                            const c64* __restrict__ noise /* [K x L_out x A] unit, NZ == 2 */,
                                                            c64* __restrict__ grid) {
  const int tid = threadIdx.x;
  int l, r;
  if (!spectral_tile_map(blockIdx.x, L_whole, A, l, r)) return;       // padding workgroup of the tile grid
  const int Q = QT ? QT : Q_rt;
  const long long colg = (long long)l + (long long)L_out * r;
  c64* dst = grid + (long long)K * colg;
  struct None_ {};
  c64 acc[16];
  spectral_echo_column<QT, NZ, 4, 256>(tid, K, Q, D + (long long)K * l, (long long)K * L_whole, steer_rq + (long long)r * Q, sig, seed, colg,
                                  NZ == 2 ? noise + (long long)K * colg : nullptr, acc, [](int) { return None_{}; },
                                  [&](int, int k, c64 v, None_) {
                                    if (k < K) {
                                      __builtin_nontemporal_store(v.re, &dst[k].re);
                                      __builtin_nontemporal_store(v.im, &dst[k].im);
                                    }
                                    return v;
                                  });
}

// 512-thread workgroups on the 8-points-per-thread transform (Fft4096W): two workgroups per CU = 16 wavefronts = four per SIMD, which
// needs <= 128 VGPRs per lane -- the second __launch_bounds__ argument is HIP's "minimum waves per execution unit (SIMD)", not CUDA's
// blocks per multiprocessor.  (The 256-thread / 16-points-per-thread form was latency-bound at two waves per SIMD: 477 us.)
// One column per workgroup: a workgroup that walks several columns (LDS tables set up once) compiles to a loop with spills and
// branches around the loads -- 0.53-0.63 ms instead of 0.40.
constexpr int kEchoRangeWavesPerSimd = 4;
// The same synthesis with the range stage of the following fft2D call (fft2D.m:37-45) applied while the column is still in
// registers: echoGrid is written once (API output + covariance input) and never re-read by the range stage; txGrid is read
// once.  HBM traffic of the launch = K L A 16 B written + K L A 16 B read (+ the CUT rows) -- the algorithmic minimum for
// monoStaticSensing's output + fft2D's range-Doppler input.  Requires nIFFT == 4096 (the FFT the registers are laid out for).
template <int QT, int NZ, int GROUP = (QT <= 1 ? 4 : 2)>   // loads in flight per thread: 2 x GROUP elements
__global__ __launch_bounds__(Fft4096W::NT, kEchoRangeWavesPerSimd) void echo_range_kernel(int K, int L_whole, int L_out, int A, int Q_rt, const c64* __restrict__ D,
                                                            const c64* __restrict__ steer_rq, double sig, uint64_t seed,
                                                            const c64* __restrict__ noise, const c64* __restrict__ tw,
                                                            c64* __restrict__ grid,
                                                            const c64* __restrict__ txg, const double* __restrict__ win_k,
                                                            const double* __restrict__ win_r, double inv_n, double sqrt_n,
                                                            int row_lo, int n_rows, c64* __restrict__ ymid) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  c64* lds = reinterpret_cast<c64*>(smem_raw);
  using FFT = Fft4096W;
  const int tid = threadIdx.x;
  FFT fft;
  const int Q = QT ? QT : Q_rt;
  int l, r;
  if (!spectral_tile_map(blockIdx.x, L_whole, A, l, r)) return;       // padding workgroup of the tile grid (before any barrier)
  const long long colg = (long long)l + (long long)L_out * r;
  fft.init_table(lds, tw, tid);                      // W512 (FFT twiddles); barrier inside
  c64* dst = grid + (long long)K * colg;
  const c64* ptx = txg + (long long)K * colg;
#pragma unroll
  for (int j = 0; j < FFT::PER; ++j) fft.x[j] = mk(0.0, 0.0);       // ifft(., nIFFT, 1) zero-pads at the end
  struct TxWin { c64 tx; double w; };
  bool live = false;                                       // any non-zero (or NaN) matched-filter sample in this column?
  spectral_echo_column<QT, NZ, GROUP, FFT::NT>(
      tid, K, Q, D + (long long)K * l, (long long)K * L_whole, steer_rq + (long long)r * Q, sig, seed, colg,
      NZ == 2 ? noise + (long long)K * colg : nullptr, fft.x,
      [&](int kc) { return TxWin{ptx[kc], win_k[kc]}; },   // txGrid sample + range window, loads unconditional
      [&](int, int k, c64 v, TxWin t) {
        if (k < K) {
          __builtin_nontemporal_store(v.re, &dst[k].re);   // echoGrid(k, l, r)
          __builtin_nontemporal_store(v.im, &dst[k].im);
        }
        c64 y = mul_conj(v, t.tx) * t.w;                    // fft2D.m:37,:43 (same order as range_kernel)
        y = k < K ? y : mk(0.0, 0.0);                       // ifft(., nIFFT, 1) zero-pads at the end
        live |= (y.re != 0.0) | (y.im != 0.0);
        return y;
      });
  c64* yd = ymid + (long long)n_rows * colg;
  // Columns of the zero-filled 'S' slots (gNBPhy.m:609-612): rx .* conj(0) is identically zero and so is its IFFT.  Decided on
  // the products themselves, so the shortcut is exact for any input (NaN / Inf products compare unequal to zero).
  if (!__syncthreads_or(live)) {
    for (int rr = tid; rr < n_rows; rr += FFT::NT) yd[rr] = mk(0.0, 0.0);
    return;
  }
  fft.init_twiddles_lds(lds, tid);
  const int blk = FFT::block_of_rows(row_lo, n_rows);     // (uniform) the CUT rows usually sit inside one 512-row block of the IFFT output
  fft.template transform<+1>(lds, tw, tid, blk);
  auto put = [&](int n, c64 v) {
    const int rr = n - row_lo;
    const double wr = win_r[n];
    if (rr >= 0 && rr < n_rows) yd[rr] = ((v * inv_n) * sqrt_n) * wr;            // fft2D.m:44-45
  };
  if (blk >= 0) fft.drain_block(put, tid, blk);
  else fft.drain(put, tid);
}

// Straight-line form of the same kernel for one or two LoS targets (the bench shape and most scenes).  The column loop above branches on
// `j < n_el` (uniform) and on `k < K` (per lane, around the echoGrid store); SIInsertWaitcnts merges the pending-memory state conservatively at
// every join, and the ISA of that form waits with `s_waitcnt vmcnt(0)` in front of EVERY element -- for the next group's loads just issued and
// for the acknowledgement of the previous element's store (gfx9: one in-order counter for loads and stores).  Here no vector-memory instruction
// sits inside a conditional: all eight elements of a thread are processed (loads at a clamped index, as before), the store is a raw buffer store
// whose descriptor ends at the column's K-th element (lanes with k >= K are dropped by the bounds check), and the waits come out as exact
// `vmcnt(N)` counts that leave the younger loads and every store in flight: 0.395 -> 0.374 ms.  With the waits exact the generator can be cut
// in two: draw group g under its own loads, issue group g + 1, consume g (the form above draws everything up front, so that the second
// group's loads were covered by the first group's four stores only): 0.374 -> 0.333-0.349 ms, 0.479 -> 0.405 ms with two targets; same bits.
// (Pointers that are loaded from between stores are NOT __restrict__: an invariant load may be sunk to its first use -- below the
// stores of the group before -- and neither sched_barrier nor a compiler fence holds it.  With three or four targets the straight-line form
// holds 2 x GROUP x (6 + 4 Q) load registers beside the generator and spills: those counts stay on the kernel above, as measured.)
// STORE = false (round 6, "lazy" echo grid: isac_mono_static_sensing_fused_dev with d_echo_grid == NULL): the echoGrid store is left out -- the grid is a function of (D, a, seed)
// that the covariance kernel re-forms for itself (cov_lazy_kernel, cov.hip), so that 0.75 GB written here and 0.75 GB read back there per CPI never cross the HBM.
template <int QT, int NZ, bool STORE = true, int GROUP = (QT <= 1 ? 4 : 2)>
__global__ __launch_bounds__(Fft4096W::NT, kEchoRangeWavesPerSimd) void echo_range_sl_kernel(int K, int L_whole, int L_out, int A, const c64* D,
                                                            const c64* __restrict__ steer_rq, double sig, uint64_t seed,
                                                            const c64* noise, const c64* __restrict__ tw,
                                                            c64* grid,
                                                            const c64* txg, const double* win_k,
                                                            const double* __restrict__ win_r, double inv_n, double sqrt_n,
                                                            int row_lo, int n_rows, c64* __restrict__ ymid) {
  constexpr bool XC = false;
  c64* const xc = nullptr;
#include "echo_range_sl_body.inc"
}

// The lazy form (STORE = false) with the cross term of the split covariance; xc [L_whole x A x QT]; 16 c64 of dynamic LDS behind Fft4096W::LDS_ELEMS.  One LoS target only:
// the two-target form of the kernel above sits at exactly 128 registers, and every placement of the cross term tried there spilled (24-388 B of scratch) -- with two LoS
// targets the range kernel stays echo_range_sl_kernel<2, 1, false, 2> and the cross term is a pass of its own in fft2D (cov_cross_kernel, cov.hip).
constexpr int kEchoXcLds = 16;
template <int QT>
__global__ __launch_bounds__(Fft4096W::NT, kEchoRangeWavesPerSimd) void echo_range_xc_kernel(int K, int L_whole, int L_out, int A, const c64* D,
                                                            const c64* __restrict__ steer_rq, double sig, uint64_t seed,
                                                            const c64* noise, const c64* __restrict__ tw,
                                                            c64* grid,
                                                            const c64* txg, const double* win_k,
                                                            const double* __restrict__ win_r, double inv_n, double sqrt_n,
                                                            int row_lo, int n_rows, c64* __restrict__ ymid, c64* __restrict__ xc,
                                                            const int* __restrict__ d_zero) {
  static_assert(QT == 1, "one LoS target (see above)");
  constexpr int NZ = 1, GROUP = 4;
  constexpr bool STORE = false, XC = true;
  // A DEAD column is decided before anything is drawn for it:  tx[k, l, r] == 0 and D[k, l] == 0 (both parts, floating-point compares: +-0 is zero, NaN and Inf are not)
  // for every k < K, and sig finite.  Its matched-filter samples are all signed zeros, so the text below would write +0.0 to its range rows, and its cross term is a sum of
  // signed zeros, which cov_assemble_kernel adds to a sum it starts at +0.0 (cov.hip): +0.0 serves.  A silent 'S' slot (isac_synth_qpsk_grid_dev zero_s_slots, gNBPhy.m:609-612)
  // is such a column for every antenna wherever the echo delays stay inside the cyclic prefix: a quarter of the bench's columns, each of which cost four Philox calls,
  // eight Box-Muller transforms and the synthesis for nothing.
  //   * The D half is ONE FLAG PER SYMBOL, d_zero[l], written by the demod_kernel launch that forms D (it has every value of the column in registers), not peek loads here:
  //     a live symbol -- three quarters of the columns -- then pays one scalar load and a uniform branch, no vector load, no barrier and no exposed latency.
  //   * Only where D[., l] is zero are the column's tx samples peeked (eight loads per thread in flight together, one workgroup-wide OR).  A column with tx != 0 there, or
  //     with tx == 0 but D != 0, takes the text below unchanged.
  {
    int l, r;
    if (!spectral_tile_map(blockIdx.x, L_whole, A, l, r)) return;       // padding workgroup of the tile grid (before any barrier)
    if (d_zero[l] != 0 && isfinite(sig)) {                              // (uniform)
      const int tid = threadIdx.x;
      const long long colg = (long long)l + (long long)L_out * r;
      const c64* ptx = txg + (long long)K * colg;
      bool nz = false;
#pragma unroll
      for (int j = 0; j < Fft4096W::PER; ++j) {
        const int k = tid + Fft4096W::NT * j;
        const c64 v = ptx[k < K ? k : K - 1];
        nz |= (v.re != 0.0) | (v.im != 0.0);
      }
      if (!__syncthreads_or(nz)) {
        c64* yd = ymid + (long long)n_rows * colg;
        for (int rr = tid; rr < n_rows; rr += Fft4096W::NT) yd[rr] = mk(0.0, 0.0);
        if (tid < QT) xc[((long long)l * A + r) * QT + tid] = mk(0.0, 0.0);
        return;
      }
    }
  }
#include "echo_range_sl_body.inc"
}

// ---------------------------------------------------------------- CP-OFDM modulator
// Placement of one call's L symbols inside larger arrays (senTx accumulation, gNBPhy.m:604-612): the grid may be a column
// range [l_off, l_off + L) of planes with `grid_cols` columns, the waveform a sample range starting at t_off of columns with
// `wave_rows` samples; `sym0` is the index of the call's first symbol inside its subframe (CP pattern, carrier.NSlot).
struct ModIo {
  long long wave_rows, t_off;
  int grid_cols, l_off, sym0, n_win;
};

template <class FFT>
__global__ __launch_bounds__(256, 2) void mod_kernel(OfdmGeom g, ModIo io, int A, int L, const c64* __restrict__ tw,
                                                     const c64* __restrict__ grid, double scale /* amplitude / nfft */,
                                                     c64* __restrict__ wave, c64* __restrict__ head /* [n_win x L x A] or null */,
                                                     const double* __restrict__ rise /* [n_win] */) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  c64* lds = reinterpret_cast<c64*>(smem_raw);
  const int tid = threadIdx.x;
  FFT fft;
  {
    const int col = blockIdx.x;                    // one (symbol, antenna) column per workgroup
    const int l = col % L, a = col / L;
    const int cp = cp_of_symbol(io.sym0 + l, g.cp_base, g.cp_long, g.sym_per_half);
    const long long s0 = symbol_start(io.sym0 + l, g.nfft, g.cp_base, g.cp_long, g.sym_per_half) -
                         symbol_start(io.sym0, g.nfft, g.cp_base, g.cp_long, g.sym_per_half);
    const c64* src = grid + (long long)g.n_sc * ((long long)(io.l_off + l) + (long long)io.grid_cols * a);
    const int half = g.n_sc / 2;
    fft.fill(
        [&](int n) {
          int kb = (n < g.nfft / 2) ? n : n - g.nfft;
          int row = kb + half;
          const bool ok = (row >= 0 && row < g.n_sc);
          c64 v = src[ok ? row : 0];                   // unconditional load, select afterwards
          return ok ? v : mk(0.0, 0.0);
        },
        tid);
    fft.init(lds, tw, tid);
    fft.template transform<+1>(lds, tw, tid);
    c64* dst = wave + io.t_off + s0 + io.wave_rows * (long long)a;
    c64* hd = head ? head + (long long)io.n_win * ((long long)l + (long long)L * a) : nullptr;
    const int h0 = g.nfft - cp - io.n_win;          // the n_win samples in front of the CP (cyclic extension), tapered by the rising edge
    fft.drain(
        [&](int m, c64 v) {
          v = v * scale;
          dst[cp + m] = v;
          if (m >= g.nfft - cp) dst[m - (g.nfft - cp)] = v;
          if (hd && m >= h0 && m < h0 + io.n_win) hd[m - h0] = v * rise[m - h0];
        },
        tid);
  }
}

// nrOFDMModulate-style windowing, second half: the last n_win samples of symbol l become  fall * own + rise * head(l + 1),
// the last symbol of the call taking the first symbol's head (the waveform of one call loops seamlessly).
__global__ __launch_bounds__(256) void mod_window_kernel(OfdmGeom g, ModIo io, int A, int L, const c64* __restrict__ head,
                                                         const double* __restrict__ rise, c64* __restrict__ wave) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long n = (long long)io.n_win * L * A;
  if (i >= n) return;
  const int w = (int)(i % io.n_win), l = (int)((i / io.n_win) % L), a = (int)(i / ((long long)io.n_win * L));
  const long long e = symbol_start(io.sym0 + l + 1, g.nfft, g.cp_base, g.cp_long, g.sym_per_half) -
                      symbol_start(io.sym0, g.nfft, g.cp_base, g.cp_long, g.sym_per_half);          // end of symbol l
  c64* p = wave + io.t_off + io.wave_rows * (long long)a + e - io.n_win + w;
  const c64 hv = head[(long long)io.n_win * ((long long)((l + 1) % L) + (long long)L * a) + w];     // already x rise
  *p = *p * rise[io.n_win - 1 - w] + hv;                                                            // fall(w) = rise(n_win - 1 - w)
}

__global__ __launch_bounds__(256) void copy_slot_kernel(const c64* __restrict__ src /* [K x L x A] */, c64* __restrict__ dst, int K, int L, int A,
                                                        int grid_cols, int l_off) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long n = (long long)K * L * A;
  if (i >= n) return;
  const long long k = i % K, l = (i / K) % L, a = i / ((long long)K * L);
  dst[k + (long long)K * ((l_off + l) + (long long)grid_cols * a)] = src ? src[i] : mk(0.0, 0.0);
}

// ---------------------------------------------------------------- synthetic QPSK grid
__global__ __launch_bounds__(256) void synth_qpsk_kernel(c64* __restrict__ grid, int K, int L, int A, uint64_t seed,
                                                         int zero_s_slots) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long n = (long long)K * L * A;
  if (i >= n) return;
  int l = (int)((i / K) % L);
  int slot = l / 14;
  c64 v = mk(0.0, 0.0);
  if (!(zero_s_slots && (slot % 4) == 3)) {
    uint32_t o[4];
    philox4x32_10((uint32_t)i, (uint32_t)((uint64_t)i >> 32), 1u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), o);
    v = mk((o[0] & 1u) ? kR2 : -kR2, (o[1] & 1u) ? kR2 : -kR2);
  }
  grid[i] = v;
}

}  // namespace isac

// ================================================================= host side
using namespace isac;

static int check_carrier(isac_ctx* ctx, const isac_carrier* c) {
  if (!c) return fail(ctx, ISAC_ERR_INVALID_ARG, "carrier is NULL");
  // (below 128 -- nrOFDMInfo's own minimum -- the normal cyclic prefix, 9 Nfft / 128 samples, is not a whole number of samples)
  if (c->nfft < 128 || c->nfft > 4096 || (c->nfft & (c->nfft - 1)))
    return fail(ctx, ISAC_ERR_UNSUPPORTED, "carrier.nfft must be a power of two in 128..4096: no integral normal cyclic prefix (144 Nfft / 2048 samples) exists below 128");
  if (c->n_sc <= 0 || c->n_sc > c->nfft || (c->n_sc & 1)) return fail(ctx, ISAC_ERR_INVALID_ARG, "carrier.n_sc invalid");
  if (c->scs_khz != 15 && c->scs_khz != 30 && c->scs_khz != 60 && c->scs_khz != 120)
    return fail(ctx, ISAC_ERR_INVALID_ARG, "carrier.scs_khz must be 15/30/60/120");
  return ISAC_OK;
}

static OfdmGeom geom_of(const isac_carrier* c) {
  Numerology n = numerology(c->nfft, c->scs_khz);
  return OfdmGeom{c->nfft, c->n_sc, n.cp_base, n.cp_long, n.sym_per_half};
}

static int whole_symbols(const OfdmGeom& g, long long T) {
  // largest L with symbol_start(L) <= T   (symbol_start(L) = end of symbol L-1)
  long long lo = 0, hi = T / g.nfft + 1;
  while (lo < hi) {
    long long mid = (lo + hi + 1) / 2;
    if (symbol_start((int)mid, g.nfft, g.cp_base, g.cp_long, g.sym_per_half) <= T) lo = mid; else hi = mid - 1;
  }
  return (int)lo;
}

extern "C" int isac_ofdm_symbol_count(const isac_carrier* carrier, int64_t T, int32_t* n_symbols) {
  if (!carrier || !n_symbols || T < 0) return ISAC_ERR_INVALID_ARG;
  *n_symbols = whole_symbols(geom_of(carrier), T);
  return ISAC_OK;
}

extern "C" int isac_ofdm_waveform_length(const isac_carrier* carrier, int32_t L, int64_t* T) {
  if (!carrier || !T || L < 0) return ISAC_ERR_INVALID_ARG;
  OfdmGeom g = geom_of(carrier);
  *T = symbol_start(L, g.nfft, g.cp_base, g.cp_long, g.sym_per_half);
  return ISAC_OK;
}

// Everything basicRadarChannel needs before samples can be synthesised: LoS compaction,
// beam-sums, coefficient vectors.  Leaves coef [Q x T], phase_rx [T], steer_rq [A x Q] in ctx.  coef_only != nullptr: the caller reads steer and, of coef, the demodulation
// windows of that carrier alone -- with one or two LoS targets the beam-sum then writes coef itself (beamsum_coef_kernel), beam / phase_rx are left as they were, and so is
// every element of coef outside those windows (beam_window.hpp).
// split != nullptr (with coef_only): the caller's covariance takes the split route (cov.hip) -- the beam-sums come out of cov_noise_beam_kernel, which forms the noise term of
// that covariance in the same launch, and coef_window_kernel writes coef from them.
struct SplitReq { int L_out; unsigned long long seed; };
static int prepare_echo(isac_ctx* ctx, const c64* d_tx, long long T, const isac_radar_channel_params* rp,
                        const uint8_t* los, int* q_out, const OfdmGeom* coef_only = nullptr, const SplitReq* split = nullptr) {
  if (!d_tx || !rp || !los) return fail(ctx, ISAC_ERR_INVALID_ARG, "NULL argument");
  if (T <= 0 || rp->n_ants <= 0 || rp->n_targets < 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "bad T / n_ants / n_targets");
  ctx->lazy.valid = false;                          // steer / coef / dgrid below are the inputs of a lazy echo grid of an earlier call: overwritten now
  if (!(rp->fs > 0)) return fail(ctx, ISAC_ERR_INVALID_ARG, "fs must be positive");
  const int A = rp->n_ants;
  const double c0 = 299792458.0;                    // physconst('Lightspeed')  basicRadarChannel.m:11
  const double lambda = c0 / rp->fc;                // :13
  const double Ts = 1.0 / rp->fs;                   // :15
  const double two_pi = 2.0 * M_PI;
  TargetTable tab{};
  std::vector<c64> steer_aq;                        // compacted LoS columns [A x Q]
  int Q = 0;
  for (int i = 0; i < rp->n_targets; ++i) {
    if (los[i] != 1) continue;                      // :40
    if (Q >= kMaxTargets) return fail(ctx, ISAC_ERR_CAPACITY, "more than 64 LoS targets");
    for (int a = 0; a < A; ++a) {
      const isac_c64 sv = rp->rx_steering[(size_t)a + (size_t)A * i];
      steer_aq.push_back(mk(sv.re, sv.im));
    }
    double path_delay = 2.0 * rp->range[i] / c0;    // :21
    tab.t[Q].shift = (long long)std::ceil(path_delay / Ts);   // :22
    double fd = 2.0 * rp->velocity[i] / lambda;     // :25
    tab.t[Q].wd = two_pi * fd;                      // 2j*pi*fd  :44
    tab.t[Q].lsf = rp->large_scale_fading[i];
    ++Q;
  }
  if (Q == 0) return fail(ctx, ISAC_ERR_NO_LOS, "no LoS target: rxWaveform is empty (basicRadarChannel.m:59,64)");
  std::vector<c64> steer_rq((size_t)A * Q);         // the same, transposed: row r holds a_q[r] at r * Q + q
  for (int q = 0; q < Q; ++q)
    for (int a = 0; a < A; ++a) steer_rq[(size_t)a * Q + q] = steer_aq[(size_t)q * A + a];
  ISAC_TRY(ensure(ctx, ctx->steer, sizeof(c64) * (size_t)A * Q * 2));
  ISAC_TRY(ensure(ctx, ctx->beam, sizeof(c64) * (size_t)Q * T));
  ISAC_TRY(ensure(ctx, ctx->coef, sizeof(c64) * (size_t)Q * T));
  ISAC_TRY(ensure(ctx, ctx->phase_rx, sizeof(c64) * (size_t)T));
  c64* d_steer_aq = (c64*)ctx->steer.p;
  const bool one_launch = coef_only && Q <= 2;      // beamsum_coef_kernel
  const bool steer_by_arg = one_launch && A * Q <= kSteerArgMax;   // ... which then takes the steering vectors as an argument and writes ctx->steer itself
  if (!steer_by_arg) {
    // pinned staging ring: the upload is truly asynchronous
    const size_t bytes = sizeof(c64) * (size_t)A * Q * 2;
    void* hst = nullptr;
    ISAC_TRY(stage_acquire(ctx, bytes, &hst));
    std::memcpy(hst, steer_aq.data(), bytes / 2);
    std::memcpy((char*)hst + bytes / 2, steer_rq.data(), bytes / 2);
    ISAC_TRY(stage_commit(ctx, d_steer_aq, bytes));
  }
  // beam-sums in tiles of up to 8 targets (tx is re-read only when Q > 8)
  const unsigned gb = cdiv(T, 256);                                   // one thread per sample (coef_kernel below)
  const unsigned gbs = (unsigned)std::min<long long>(gb, 1024);        // beam-sum: long-lived workgroups (sweep: profiles/r04_beamsum_sweep.txt)
  timeline_mark(ctx, 0, ctx->stream);
  const double w = two_pi * rp->fc;                 // 2j*pi*fc  :30,:73
  if (one_launch) {                                 // the beam-sum writes coef itself, inside the demodulation windows; beam and phase_rx stay unwritten (the caller reads neither)
    long long d_min = tab.t[0].shift, d_max = d_min;
    for (int q = 1; q < Q; ++q) { d_min = std::min(d_min, tab.t[q].shift); d_max = std::max(d_max, tab.t[q].shift); }
    const OfdmGeom& g = *coef_only;
    constexpr long long kSpan = 1LL << 38;          // T + d_max in 256-sample units is an int
    if (T >= kSpan || d_max >= kSpan || d_min <= -kSpan) return fail(ctx, ISAC_ERR_CAPACITY, "waveform or target delay beyond the beam-sum's unit count");
    const BeamWindow bw = beam_window(g.nfft, g.cp_base, g.cp_long, g.sym_per_half, whole_symbols(g, T), T, d_min, d_max);
    const unsigned gbu = (unsigned)std::max<long long>(1, std::min<long long>(bw_units(bw), 1024));   // long-lived workgroups, as above
    if (split) {
      const LazySplitFront f{d_tx, T, A, Q, steer_by_arg ? steer_aq.data() : nullptr, bw, g.n_sc, whole_symbols(g, T), split->L_out, split->seed};
      ISAC_TRY(isac_cov_noise_beam_on(ctx, ctx->stream, f));
      timeline_mark(ctx, 1, ctx->stream);
      auto coefs = [&](auto qc) {
        constexpr int QT = decltype(qc)::value;
        CoefTargets<QT> ct;
        for (int q = 0; q < QT; ++q) ct.t[q] = tab.t[q];
        hipLaunchKernelGGL((coef_window_kernel<QT>), dim3((unsigned)bw_units(bw)), dim3(256), 0, ctx->stream, (const c64*)ctx->beam.p, T, bw, ct, w, Ts, (c64*)ctx->coef.p);
      };
      if (Q == 1) coefs(std::integral_constant<int, 1>{});
      else coefs(std::integral_constant<int, 2>{});
      ISAC_HIP(hipGetLastError());
      *q_out = Q;
      return ISAC_OK;
    }
    SteerArg sa{};
    if (steer_by_arg) std::memcpy(sa.v, steer_aq.data(), sizeof(c64) * (size_t)A * Q);
    auto launch = [&](auto qc) {
      constexpr int QT = decltype(qc)::value;
      CoefTargets<QT> ct;
      for (int q = 0; q < QT; ++q) ct.t[q] = tab.t[q];
      hipLaunchKernelGGL((beamsum_coef_kernel<QT, 32>), dim3(gbu), dim3(256), sizeof(c64) * A * QT, ctx->stream, d_tx, T, A, steer_by_arg ? nullptr : (const c64*)d_steer_aq, sa,
                         d_steer_aq, bw, ct, w, Ts, (c64*)ctx->coef.p);
    };
    if (Q == 1) launch(std::integral_constant<int, 1>{});
    else launch(std::integral_constant<int, 2>{});
    ISAC_HIP(hipGetLastError());
    timeline_mark(ctx, 1, ctx->stream);
    *q_out = Q;
    return ISAC_OK;
  }
#define ISAC_BEAMSUM(QT) \
  hipLaunchKernelGGL((beamsum_kernel<QT, (QT <= 2 ? 32 : 8)>), dim3(gbs), dim3(256), sizeof(c64) * A * QT, ctx->stream, d_tx, T, A, st, bm)
  for (int q0 = 0; q0 < Q;) {
    int rem = Q - q0;
    const c64* st = d_steer_aq + (size_t)q0 * A;
    c64* bm = (c64*)ctx->beam.p + (size_t)q0 * T;
    if (rem >= 8) { ISAC_BEAMSUM(8); q0 += 8; }
    else if (rem >= 4) { ISAC_BEAMSUM(4); q0 += 4; }
    else if (rem >= 2) { ISAC_BEAMSUM(2); q0 += 2; }
    else { ISAC_BEAMSUM(1); q0 += 1; }
  }
#undef ISAC_BEAMSUM
  timeline_mark(ctx, 1, ctx->stream);
  hipLaunchKernelGGL(coef_kernel, dim3(gb), dim3(256), 0, ctx->stream, (const c64*)ctx->beam.p, T, Q, tab, w, Ts,
                     (c64*)ctx->coef.p, (c64*)ctx->phase_rx.p);
  ISAC_HIP(hipGetLastError());
  *q_out = Q;
  return ISAC_OK;
}

// rxWaveform [T x A] from what prepare_echo / isac_path_coefs_on left in the context (coef [Q x T], phase_rx [T], steer): the tail of both time-domain channel calls
static int waveform_from_coefs(isac_ctx* ctx, long long T, int A, int Q, double n0, int noise_mode, const c64* d_noise_unit, uint64_t seed, c64* d_rx_wave) {
  const double n0s = std::sqrt(n0 / 2.0);           // basicRadarChannel.m:67
  hipLaunchKernelGGL(radar_waveform_kernel, dim3(cdiv(T, 256), A), dim3(256), 0, ctx->stream, T, A, Q,
                     (const c64*)ctx->coef.p, (const c64*)ctx->steer.p + (size_t)A * Q, (const c64*)ctx->phase_rx.p,
                     noise_mode, d_noise_unit, n0s, seed, d_rx_wave);
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}

extern "C" int isac_basic_radar_channel_dev(isac_ctx* ctx, const isac_c64* d_tx_wave, int64_t T,
                                            const isac_radar_channel_params* rp, const uint8_t* los, int noise_mode,
                                            const isac_c64* d_noise_unit, uint64_t seed, isac_c64* d_rx_wave) {
  ISAC_ENTER(ctx);
  if (!d_rx_wave) return fail(ctx, ISAC_ERR_INVALID_ARG, "rx_wave is NULL");
  if (noise_mode == ISAC_NOISE_INJECTED && !d_noise_unit) return fail(ctx, ISAC_ERR_INVALID_ARG, "noise buffer missing");
  if (noise_mode < ISAC_NOISE_NONE || noise_mode > ISAC_NOISE_PHILOX)
    return fail(ctx, ISAC_ERR_INVALID_ARG, "basicRadarChannel returns a time-domain waveform: noise modes NONE / INJECTED / PHILOX only");
  int Q = 0;
  ISAC_TRY(prepare_echo(ctx, (const c64*)d_tx_wave, T, rp, los, &Q));
  return waveform_from_coefs(ctx, T, rp->n_ants, Q, rp->n0, noise_mode, (const c64*)d_noise_unit, seed, (c64*)d_rx_wave);
}

// f(std::integral_constant<int, Q>) for a LoS target count the kernels have as a compile-time constant (1..MAXQ), f(<0>) -- the run-time count -- for any other
template <int MAXQ, class F>
static int echo_dispatch(int Q, F&& f) {
  if constexpr (MAXQ > 0)
    if (Q != MAXQ) return echo_dispatch<MAXQ - 1>(Q, f);
  return f(std::integral_constant<int, MAXQ>{});
}

// monoStaticSensing.m:19-21: the grid has at least the transmit grid's symbol count (the caller zero-fills a grid that is wider than the waveform)
static int padded_symbols(int L_whole, int tx_dim_l, int32_t* l_out) {
  const int L_out = L_whole < tx_dim_l ? tx_dim_l : L_whole;
  if (l_out) *l_out = L_out;
  return L_out;
}

template <class FFT, bool SYNTH, int QT = 0>
static int launch_demod(isac_ctx* ctx, const OfdmGeom& g, long long T, int A, int L_whole, int L_out, const c64* tw, int Q,
                        int noise_mode, const c64* noise, double n0s, uint64_t seed, const c64* wave, c64* grid, int* zero_flag = nullptr) {
  size_t lds = sizeof(c64) * (FFT::LDS_ELEMS + kLogTabSize);
  const c64* logtab = nullptr;
  ISAC_TRY(isac_get_logtab(ctx, &logtab));
  auto kern = demod_kernel<FFT, SYNTH, QT>;
  ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(kern), lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)(L_whole * A)) /* one column per workgroup (two 72 KB workgroups per CU) */, dim3(256), lds, ctx->stream, g, T, A, L_whole, L_out, tw, Q,
                     (const c64*)ctx->coef.p, SYNTH ? (const c64*)ctx->steer.p + (size_t)A * Q : nullptr,
                     (const c64*)ctx->phase_rx.p, noise_mode, noise, n0s, seed, wave, grid, logtab, zero_flag);
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}

// ---- spectral noise modes: per-target demodulated coefficient grids D [K x L_whole x Q] (the coefficient vectors
// coef [Q x T] are, byte for byte, a [T x Q] waveform), then one synthesis kernel.
static int* dgrid_zero_flags(isac_ctx* ctx, int K, int L_whole, int Q) { return reinterpret_cast<int*>((c64*)ctx->dgrid.p + (size_t)K * L_whole * Q); }

// D = OFDM-demodulate(coef as a [T x Q] waveform) -> ctx->dgrid
static int demod_coefs(isac_ctx* ctx, const OfdmGeom& g, long long T, int Q, int L_whole) {
  // D, and behind it one zero flag per column of D (demod_kernel's zero_flag: the D half of echo_range_xc_kernel's dead-column test)
  ISAC_TRY(ensure(ctx, ctx->dgrid, sizeof(c64) * (size_t)g.n_sc * L_whole * Q + sizeof(int) * (size_t)L_whole * Q));
  const c64* tw = nullptr;
  ISAC_TRY(isac_get_twiddles(ctx, g.nfft, &tw));
  ISAC_FFT_DISPATCH(g.nfft, ISAC_TRY((launch_demod<FFT, false>(ctx, g, T, Q, L_whole, L_whole, tw, 0, 0, nullptr, 0.0, 0,
                                                               (const c64*)ctx->coef.p, (c64*)ctx->dgrid.p, dgrid_zero_flags(ctx, g.n_sc, L_whole, Q)))));
  return ISAC_OK;
}

static int spectral_prepare(isac_ctx* ctx, const c64* d_tx, long long T, const isac_radar_channel_params* rp, const uint8_t* los,
                            const OfdmGeom& g, int* q_out, int* l_whole_out, bool coef_only = false, const SplitReq* split = nullptr) {
  int Q = 0;
  ISAC_TRY(prepare_echo(ctx, d_tx, T, rp, los, &Q, coef_only ? &g : nullptr, split));       // monoStaticSensing.m:13
  const int L_whole = whole_symbols(g, T);
  if (L_whole <= 0) return fail(ctx, ISAC_ERR_SHORT_WAVEFORM, "waveform shorter than one OFDM symbol");
  ISAC_TRY(demod_coefs(ctx, g, T, Q, L_whole));
  *q_out = Q;
  *l_whole_out = L_whole;
  return ISAC_OK;
}

static bool spectral_mode(int noise_mode) { return noise_mode == ISAC_NOISE_PHILOX_SPECTRAL || noise_mode == ISAC_NOISE_INJECTED_SPECTRAL; }

template <int QT>
static int launch_echo_spectral(isac_ctx* ctx, const OfdmGeom& g, int A, int L_whole, int L_out, int Q, int noise_mode,
                                const c64* noise, double sig, uint64_t seed, c64* grid) {
  const dim3 gr((unsigned)spectral_grid_size(L_whole, A)), bl(256);
  const c64* D = (const c64*)ctx->dgrid.p;
  const c64* srq = (const c64*)ctx->steer.p + (size_t)A * Q;
  auto kern = noise_mode == ISAC_NOISE_PHILOX_SPECTRAL ? echo_spectral_kernel<QT, 1> : noise_mode == ISAC_NOISE_INJECTED_SPECTRAL ? echo_spectral_kernel<QT, 2> : echo_spectral_kernel<QT, 0>;
  hipLaunchKernelGGL(kern, gr, bl, 0, ctx->stream, g.n_sc, L_whole, L_out, A, Q, D, srq, sig, seed, noise, grid);
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}

// One launch of a fused synthesis + range kernel (echo_range_kernel / echo_range_sl_kernel: Fft4096W workgroups, one per tile-map slot)
template <class Kern, class... Args>
static int launch_echo_range(isac_ctx* ctx, Kern kern, int L_whole, int A, size_t lds_extra, Args... args) {
  const size_t lds = sizeof(c64) * Fft4096W::LDS_ELEMS + lds_extra;
  ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(kern), lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)spectral_grid_size(L_whole, A)), dim3(Fft4096W::NT), lds, ctx->stream, args...);
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}

// echoGrid [n_sc x L_out x A] from what prepare_echo / isac_path_coefs_on left in the context (coef [Q x T], phase_rx [T], steer): OFDM demodulation of the synthesised
// samples (monoStaticSensing.m:16), or -- spectral noise modes -- of the Q coefficient vectors and the spectral synthesis; zero-padding up to tx_dim_l symbols (:19-21).
// The tail of isac_mono_static_sensing_dev and isac_multi_static_sensing_dev.
static int grid_from_coefs(isac_ctx* ctx, const OfdmGeom& g, long long T, int A, int Q, double n0, int tx_dim_l, int noise_mode, const c64* d_noise,
                           uint64_t seed, c64* d_grid, int32_t* l_out, const PathFrac* frac = nullptr /* spectral modes: fractional delays of the Q paths (include/isac_subsample.h) */) {
  const int L_whole = whole_symbols(g, T);
  if (L_whole <= 0) return fail(ctx, ISAC_ERR_SHORT_WAVEFORM, "waveform shorter than one OFDM symbol");
  if (spectral_mode(noise_mode)) ISAC_TRY(demod_coefs(ctx, g, T, Q, L_whole));
  if (frac) ISAC_TRY(isac_path_frac_ramp_on(ctx, ctx->stream, *frac, g.n_sc, g.nfft, L_whole, Q));
  const int L_out = padded_symbols(L_whole, tx_dim_l, l_out);
  if (L_out > L_whole) ISAC_HIP(hipMemsetAsync(d_grid, 0, sizeof(c64) * (size_t)g.n_sc * L_out * A, ctx->stream));
  if (spectral_mode(noise_mode)) {
    const double sig = std::sqrt(n0 / 2.0) * std::sqrt((double)g.nfft);              // basicRadarChannel.m:67 through the unscaled FFT
    return echo_dispatch<4>(Q, [&](auto qc) { return launch_echo_spectral<decltype(qc)::value>(ctx, g, A, L_whole, L_out, Q, noise_mode, d_noise, sig, seed, d_grid); });
  }
  const c64* tw = nullptr;
  ISAC_TRY(isac_get_twiddles(ctx, g.nfft, &tw));
  const double n0s = std::sqrt(n0 / 2.0);
  if (g.nfft == 4096)      // the target count as a compile-time constant where the kernel has one (1..4)
    return echo_dispatch<4>(Q, [&](auto qc) {
      return launch_demod<Fft4096, true, decltype(qc)::value>(ctx, g, T, A, L_whole, L_out, tw, Q, noise_mode, d_noise, n0s, seed, nullptr, d_grid);
    });
  ISAC_FFT_DISPATCH(g.nfft, ISAC_TRY((launch_demod<FFT, true>(ctx, g, T, A, L_whole, L_out, tw, Q, noise_mode, d_noise, n0s, seed, nullptr, d_grid))));
  return ISAC_OK;
}

extern "C" int isac_mono_static_sensing_dev(isac_ctx* ctx, const isac_c64* d_tx_wave, int64_t T, int32_t tx_dim_l,
                                            const isac_carrier* carrier, const isac_radar_channel_params* rp,
                                            const uint8_t* los, int noise_mode, const isac_c64* d_noise_unit,
                                            uint64_t seed, isac_c64* d_echo_grid, int32_t* l_out) {
  ISAC_ENTER(ctx);
  ctx->range_cache.valid = false;
  ISAC_TRY(check_carrier(ctx, carrier));
  if (!d_echo_grid) return fail(ctx, ISAC_ERR_INVALID_ARG, "echo_grid is NULL");
  if ((noise_mode == ISAC_NOISE_INJECTED || noise_mode == ISAC_NOISE_INJECTED_SPECTRAL) && !d_noise_unit)
    return fail(ctx, ISAC_ERR_INVALID_ARG, "noise buffer missing");
  if (noise_mode < ISAC_NOISE_NONE || noise_mode > ISAC_NOISE_INJECTED_SPECTRAL) return fail(ctx, ISAC_ERR_INVALID_ARG, "unknown noise mode");
  int Q = 0;
  ISAC_TRY(prepare_echo(ctx, (const c64*)d_tx_wave, T, rp, los, &Q));   // monoStaticSensing.m:13
  return grid_from_coefs(ctx, geom_of(carrier), T, rp->n_ants, Q, rp->n0, tx_dim_l, noise_mode, (const c64*)d_noise_unit, seed, (c64*)d_echo_grid, l_out);
}

// ---------------------------------------------------------------- multi-static echo (include/isac_multistatic.h): paths from several source arrays.  The checks and the
// two entry points; the coefficient vectors: multistatic.hip; everything behind them: the tails above.
static int check_paths(isac_ctx* ctx, const PathCoefJob& j, int n_sources) {
  if (!j.d_tx || !j.n_ants_src) return fail(ctx, ISAC_ERR_INVALID_ARG, "NULL argument");
  if (j.T <= 0 || j.n_ants <= 0 || n_sources <= 0 || j.n_paths < 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "bad T / n_ants / n_sources / n_paths");
  if (!(j.fs > 0)) return fail(ctx, ISAC_ERR_INVALID_ARG, "fs must be positive");
  if (j.n_paths == 0) return fail(ctx, ISAC_ERR_NO_LOS, "no path: rxWaveform is empty (basicRadarChannel.m:59,64)");
  if (j.n_paths > ISAC_MULTISTATIC_MAX_PATHS) return fail(ctx, ISAC_ERR_CAPACITY, "more than 64 paths");
  if (n_sources > ISAC_MULTISTATIC_MAX_SOURCES) return fail(ctx, ISAC_ERR_CAPACITY, "more than 32 sources");
  if (j.n_ants > ISAC_MULTISTATIC_MAX_ANTS) return fail(ctx, ISAC_ERR_CAPACITY, "more than 256 receive elements");
  if (!j.path_source || !j.path_shift || !j.path_doppler_hz || !j.path_gain || !j.path_tx_steering || !j.path_rx_steering) return fail(ctx, ISAC_ERR_INVALID_ARG, "NULL argument");
  for (int p = 0; p < j.n_paths; ++p) {
    const int s = j.path_source[p];
    if (s < 0 || s >= n_sources) return fail(ctx, ISAC_ERR_INVALID_ARG, "path_source outside 0 .. n_sources - 1");
    if (j.path_shift[p] < 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "negative path_shift");
    if (!j.d_tx[s] || j.n_ants_src[s] <= 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "a path names a source without a waveform");
    if (j.n_ants_src[s] > ISAC_MULTISTATIC_MAX_ANTS) return fail(ctx, ISAC_ERR_CAPACITY, "more than 256 elements on a source array");
  }
  return ISAC_OK;
}

extern "C" int isac_multi_static_channel_dev(isac_ctx* ctx, const isac_c64* const* d_tx_waves, const int32_t* n_ants_src, int32_t n_sources, int64_t T, double fc, double fs,
                                             double n0, int32_t n_ants, int32_t n_paths, const int32_t* path_source, const int64_t* path_shift, const double* path_doppler_hz,
                                             const double* path_gain, const isac_c64* path_tx_steering, const isac_c64* path_rx_steering, int noise_mode,
                                             const isac_c64* d_noise_unit, uint64_t seed, isac_c64* d_rx_wave) {
  ISAC_ENTER(ctx);
  if (!d_rx_wave) return fail(ctx, ISAC_ERR_INVALID_ARG, "rx_wave is NULL");
  if (noise_mode == ISAC_NOISE_INJECTED && !d_noise_unit) return fail(ctx, ISAC_ERR_INVALID_ARG, "noise buffer missing");
  if (noise_mode < ISAC_NOISE_NONE || noise_mode > ISAC_NOISE_PHILOX)
    return fail(ctx, ISAC_ERR_INVALID_ARG, "a time-domain waveform: noise modes NONE / INJECTED / PHILOX only");
  const PathCoefJob j{(const c64* const*)d_tx_waves, n_ants_src, T, fc, fs, n_ants, n_paths, path_source, path_shift, path_doppler_hz, path_gain, path_tx_steering, path_rx_steering};
  ISAC_TRY(check_paths(ctx, j, n_sources));
  ctx->range_cache.valid = false;
  ctx->lazy.valid = false;                          // steer / coef below are the inputs of a lazy echo grid of an earlier call
  ISAC_TRY(isac_path_coefs_on(ctx, ctx->stream, j));
  return waveform_from_coefs(ctx, T, n_ants, n_paths, n0, noise_mode, (const c64*)d_noise_unit, seed, (c64*)d_rx_wave);
}

// The body of isac_multi_static_sensing_dev and isac_multi_static_sensing_frac_dev (include/isac_subsample.h); path_frac == NULL: the former
static int multi_static_sensing(isac_ctx* ctx, const isac_c64* const* d_tx_waves, const int32_t* n_ants_src, int32_t n_sources, int64_t T, double fc, double fs,
                                double n0, int32_t n_ants, int32_t n_paths, const int32_t* path_source, const int64_t* path_shift, const double* path_frac, const double* path_doppler_hz,
                                const double* path_gain, const isac_c64* path_tx_steering, const isac_c64* path_rx_steering, int noise_mode,
                                const isac_c64* d_noise_unit, uint64_t seed, int32_t tx_dim_l, const isac_carrier* carrier, isac_c64* d_echo_grid, int32_t* l_out) {
  ISAC_ENTER(ctx);
  ISAC_TRY(check_carrier(ctx, carrier));
  if (!d_echo_grid) return fail(ctx, ISAC_ERR_INVALID_ARG, "echo_grid is NULL");
  if ((noise_mode == ISAC_NOISE_INJECTED || noise_mode == ISAC_NOISE_INJECTED_SPECTRAL) && !d_noise_unit)
    return fail(ctx, ISAC_ERR_INVALID_ARG, "noise buffer missing");
  if (noise_mode < ISAC_NOISE_NONE || noise_mode > ISAC_NOISE_INJECTED_SPECTRAL) return fail(ctx, ISAC_ERR_INVALID_ARG, "unknown noise mode");
  const PathCoefJob j{(const c64* const*)d_tx_waves, n_ants_src, T, fc, fs, n_ants, n_paths, path_source, path_shift, path_doppler_hz, path_gain, path_tx_steering, path_rx_steering};
  ISAC_TRY(check_paths(ctx, j, n_sources));
  bool any_frac = false;                                                 // include/isac_subsample.h: every delta in [0, 1); a non-zero one needs a spectral mode
  for (int p = 0; path_frac && p < n_paths; ++p) {
    if (!(path_frac[p] >= 0.0 && path_frac[p] < 1.0)) return fail(ctx, ISAC_ERR_INVALID_ARG, "a path_frac outside [0, 1) or not finite");
    any_frac |= path_frac[p] != 0.0;
  }
  if (any_frac && !spectral_mode(noise_mode)) return fail(ctx, ISAC_ERR_UNSUPPORTED, "a fractional path delay needs a spectral noise mode: the waveform route would need an interpolation filter");
  const OfdmGeom g = geom_of(carrier);
  if (whole_symbols(g, T) <= 0) return fail(ctx, ISAC_ERR_SHORT_WAVEFORM, "waveform shorter than one OFDM symbol");   // (before any launch: a refused call writes nothing)
  ctx->range_cache.valid = false;
  ctx->lazy.valid = false;
  ISAC_TRY(isac_path_coefs_on(ctx, ctx->stream, j));
  const PathFrac pf{path_frac, fc, fs};
  return grid_from_coefs(ctx, g, T, n_ants, n_paths, n0, tx_dim_l, noise_mode, (const c64*)d_noise_unit, seed, (c64*)d_echo_grid, l_out, any_frac ? &pf : nullptr);
}

extern "C" int isac_multi_static_sensing_dev(isac_ctx* ctx, const isac_c64* const* d_tx_waves, const int32_t* n_ants_src, int32_t n_sources, int64_t T, double fc, double fs,
                                             double n0, int32_t n_ants, int32_t n_paths, const int32_t* path_source, const int64_t* path_shift, const double* path_doppler_hz,
                                             const double* path_gain, const isac_c64* path_tx_steering, const isac_c64* path_rx_steering, int noise_mode,
                                             const isac_c64* d_noise_unit, uint64_t seed, int32_t tx_dim_l, const isac_carrier* carrier, isac_c64* d_echo_grid, int32_t* l_out) {
  return multi_static_sensing(ctx, d_tx_waves, n_ants_src, n_sources, T, fc, fs, n0, n_ants, n_paths, path_source, path_shift, nullptr, path_doppler_hz, path_gain, path_tx_steering,
                              path_rx_steering, noise_mode, d_noise_unit, seed, tx_dim_l, carrier, d_echo_grid, l_out);
}

extern "C" int isac_multi_static_sensing_frac_dev(isac_ctx* ctx, const isac_c64* const* d_tx_waves, const int32_t* n_ants_src, int32_t n_sources, int64_t T, double fc, double fs,
                                                  double n0, int32_t n_ants, int32_t n_paths, const int32_t* path_source, const int64_t* path_shift, const double* path_frac,
                                                  const double* path_doppler_hz, const double* path_gain, const isac_c64* path_tx_steering, const isac_c64* path_rx_steering,
                                                  int noise_mode, const isac_c64* d_noise_unit, uint64_t seed, int32_t tx_dim_l, const isac_carrier* carrier, isac_c64* d_echo_grid,
                                                  int32_t* l_out) {
  return multi_static_sensing(ctx, d_tx_waves, n_ants_src, n_sources, T, fc, fs, n0, n_ants, n_paths, path_source, path_shift, path_frac, path_doppler_hz, path_gain, path_tx_steering,
                              path_rx_steering, noise_mode, d_noise_unit, seed, tx_dim_l, carrier, d_echo_grid, l_out);
}

extern "C" int isac_mono_static_sensing_fused_dev(isac_ctx* ctx, const isac_c64* d_tx_wave, int64_t T, int32_t tx_dim_l,
                                                  const isac_carrier* carrier, const isac_radar_channel_params* rp,
                                                  const uint8_t* los, int noise_mode, const isac_c64* d_noise_unit,
                                                  uint64_t seed, isac_c64* d_echo_grid, int32_t* l_out,
                                                  const isac_est_params* ep, const isac_cfar_config* cf,
                                                  const isac_c64* d_tx_grid) {
  ISAC_ENTER(ctx);
  ctx->range_cache.valid = false;
  ctx->lazy.valid = false;
  ISAC_TRY(check_carrier(ctx, carrier));
  if (!ep || !cf || !d_tx_grid || !rp) return fail(ctx, ISAC_ERR_INVALID_ARG, "NULL argument");
  if (noise_mode == ISAC_NOISE_INJECTED && !d_noise_unit) return fail(ctx, ISAC_ERR_INVALID_ARG, "noise buffer missing");
  OfdmGeom g = geom_of(carrier);
  CutRows cr;
  const bool rows_ok = cut_rows_ok(ep, cf, &cr) && cf->row1 >= cf->row0;
  const bool fusable = g.nfft == 4096 && ep->n_ifft == g.nfft && rows_ok;
  // d_echo_grid == NULL: the echo grid stays inside the context (LazyEcho, isac_common.hpp).  Where the kernels can re-form it -- the fused spectral route with Philox noise,
  // 49..64 antennas, one or two LoS targets -- nothing is stored at all; every other shape gets a context-owned buffer and runs exactly as with a caller's array.
  const bool lazy = d_echo_grid == nullptr;
  bool lazy_native = false;
  if (lazy) {
    int n_los = 0;
    if (!los) return fail(ctx, ISAC_ERR_INVALID_ARG, "NULL argument");
    for (int i = 0; i < rp->n_targets; ++i) n_los += los[i] == 1;
    lazy_native = fusable && noise_mode == ISAC_NOISE_PHILOX_SPECTRAL && rp->n_ants > 48 && rp->n_ants <= 64 && n_los >= 1 && n_los <= 2;
    if (!lazy_native) {
      int32_t lw = 0;
      ISAC_TRY(isac_ofdm_symbol_count(carrier, T, &lw));
      const int lo_ = padded_symbols(lw, tx_dim_l, nullptr);
      if (lo_ <= 0) return fail(ctx, ISAC_ERR_SHORT_WAVEFORM, "waveform shorter than one OFDM symbol");
      ISAC_TRY(ensure(ctx, ctx->echo_own, sizeof(c64) * (size_t)g.n_sc * lo_ * rp->n_ants));
      d_echo_grid = (isac_c64*)ctx->echo_own.p;
    }
  }
  // No fused kernel: the plain synthesis, then (cache_rows) the range stage of the following fft2D launched right behind it -- the contract (stage results cached for
  // isac_fft2d_submit_cached_dev) holds for every carrier and noise mode.
  auto plain_then_range = [&](bool cache_rows) -> int {
    int32_t lo = 0;
    ISAC_TRY(isac_mono_static_sensing_dev(ctx, d_tx_wave, T, tx_dim_l, carrier, rp, los, noise_mode, d_noise_unit, seed, d_echo_grid, &lo));
    if (l_out) *l_out = lo;
    if (lazy) ctx->lazy.set_owned(g.n_sc, lo, rp->n_ants);
    if (!cache_rows) return ISAC_OK;
    return isac_range_stage_into_cache(ctx, ep, cf, (const c64*)d_echo_grid, (const c64*)d_tx_grid, g.n_sc, lo, rp->n_ants);
  };
  // other numerologies (Nfft != 4096 or nIFFT != Nfft).  A CUT window that leaves the map is fft2D's error to report: nothing is cached then.
  if (!fusable) return plain_then_range(rows_ok && ep->n_ifft >= g.n_sc && (ep->n_ifft & (ep->n_ifft - 1)) == 0);
  if (noise_mode < ISAC_NOISE_NONE || noise_mode > ISAC_NOISE_INJECTED_SPECTRAL) return fail(ctx, ISAC_ERR_INVALID_ARG, "unknown noise mode");
  if (noise_mode == ISAC_NOISE_INJECTED_SPECTRAL && !d_noise_unit) return fail(ctx, ISAC_ERR_INVALID_ARG, "noise buffer missing");
  // time-domain noise modes (NONE / INJECTED / PHILOX per sample): the per-antenna demodulation kernel and the range kernel, no fused kernel (the 256-thread demodulator
  // and the 512-thread range transform do not share a workgroup shape; the fused time-domain kernel of round 1 was slower than the two launches anyway).
  if (!spectral_mode(noise_mode)) return plain_then_range(true);
  int Q = 0, L_whole = 0;
  // (tried in round 6 and removed: the front of the call -- beam-sum, coefficient vectors, Q x L demodulation FFTs -- on a lowest-priority third stream per context, so that it
  //  would yield to the compute-bound kernels of the CPIs ahead: 24 streams on 16 hardware queues collapse the pipelined rate to 4-5 k slots/s whatever GPU_MAX_HW_QUEUES says,
  //  and with 4-5 contexts (12-15 streams) it is 7-15 % slower than two streams per context; profiles/r06_lazy_first_measurements.txt)
  // (coef_only: this route reads coef and steer alone; isac_mono_static_sensing_dev keeps beamsum_kernel + coef_kernel and is the in-tree reference of the one-launch form)
  // the covariance of a native lazy grid on the split route (ISAC_LAZY_COV_SPLIT, cov.hip): its noise term is formed at the head of the call, beside the beam-sum
  const int lw_pre = whole_symbols(g, T);
  const SplitReq sreq{padded_symbols(lw_pre, tx_dim_l, nullptr), seed};
  const bool split = lazy_native && ctx->lazy_cov_route == 0 && lw_pre > 0 && isac_lazy_split_ok(T, g.n_sc, lw_pre);
  ISAC_TRY(spectral_prepare(ctx, (const c64*)d_tx_wave, T, rp, los, g, &Q, &L_whole, true, split ? &sreq : nullptr));
  const int A = rp->n_ants, row_lo = cr.row_lo, nr = cr.nr;
  const int L_out = padded_symbols(L_whole, tx_dim_l, l_out);
  if (split) ISAC_TRY(ensure(ctx, ctx->cov_xc, sizeof(c64) * lazy_xc_total(L_whole, A, Q)));
  ctx->tgt.drop();                                     // the fused kernel rewrites the range rows isac_fft2d_get_targets reads
  ISAC_TRY(ensure(ctx, ctx->ymid, sizeof(c64) * (size_t)nr * L_out * A));
  if (L_out > L_whole) {
    if (!lazy_native) ISAC_HIP(hipMemsetAsync(d_echo_grid, 0, sizeof(c64) * (size_t)g.n_sc * L_out * A, ctx->stream));
    ISAC_HIP(hipMemsetAsync(ctx->ymid.p, 0, sizeof(c64) * (size_t)nr * L_out * A, ctx->stream));
  }
  const c64* tw = nullptr;
  const double *wk = nullptr, *wr = nullptr;
  ISAC_TRY(isac_get_w512_pack(ctx, &tw));            // Fft4096W's packed LDS tables (the fused kernel needs nothing else of the 4096 table)
  ISAC_TRY(isac_get_windows(ctx, g.n_sc, ep->n_ifft, &wk, &wr));
  const double sig = std::sqrt(rp->n0 / 2.0) * std::sqrt((double)g.nfft);
  if (!ctx->profile_cov) ISAC_TRY(profile_begin(ctx));   // isac_profile_*: brackets exactly the fused kernel below
  timeline_mark(ctx, 2, ctx->stream);
  // the two kernels' argument lists differ in the run-time target count `q_rt` alone (the straight-line form has none)
  auto launch = [&](auto kern, auto... q_rt) {
    return launch_echo_range(ctx, kern, L_whole, A, (size_t)0, g.n_sc, L_whole, L_out, A, q_rt..., (const c64*)ctx->dgrid.p, (const c64*)ctx->steer.p + (size_t)A * Q, sig, seed,
                             (const c64*)d_noise_unit, tw, (c64*)d_echo_grid, (const c64*)d_tx_grid, wk, wr, 1.0 / ep->n_ifft, std::sqrt((double)ep->n_ifft), row_lo, nr,
                             (c64*)ctx->ymid.p);
  };
  const bool philox = noise_mode == ISAC_NOISE_PHILOX_SPECTRAL;
  ISAC_TRY(echo_dispatch<4>(Q, [&](auto qc) {
    constexpr int QT = decltype(qc)::value;
    if constexpr (QT == 1 || QT == 2) {     // the straight-line form; lazy_native: without the echoGrid store (d_echo_grid is NULL, the noise is Philox)
      if constexpr (QT == 1)
        if (split)                          // ... and with the cross term of the split covariance (the one extra argument; two targets: cov_cross_kernel forms it in fft2D)
          return launch_echo_range(ctx, echo_range_xc_kernel<QT>, L_whole, A, sizeof(c64) * kEchoXcLds, g.n_sc, L_whole, L_out, A, (const c64*)ctx->dgrid.p, (const c64*)ctx->steer.p + (size_t)A * Q, sig, seed,
                                 (const c64*)d_noise_unit, tw, (c64*)d_echo_grid, (const c64*)d_tx_grid, wk, wr, 1.0 / ep->n_ifft, std::sqrt((double)ep->n_ifft), row_lo, nr,
                                 (c64*)ctx->ymid.p, (c64*)ctx->cov_xc.p, (const int*)dgrid_zero_flags(ctx, g.n_sc, L_whole, Q));
      return launch(lazy_native ? echo_range_sl_kernel<QT, 1, false> : philox ? echo_range_sl_kernel<QT, 1> : echo_range_sl_kernel<QT, 2>);
    } else
      return launch(philox ? echo_range_kernel<QT, 1> : echo_range_kernel<QT, 2>, Q);
  }));
  if (!ctx->profile_cov) ISAC_TRY(profile_end(ctx));
  timeline_mark(ctx, 3, ctx->stream);
  ctx->range_cache.set(d_echo_grid, d_tx_grid, g.n_sc, L_out, A, ep->n_ifft, row_lo, nr);   // (rx == NULL: the native lazy grid)
  if (lazy_native) { ctx->lazy.set_native(g.n_sc, L_whole, L_out, A, Q, sig, seed); ctx->lazy.split = split; }
  else if (lazy) ctx->lazy.set_owned(g.n_sc, L_out, A);
  return ISAC_OK;
}

// The lazy echo grid of the last fused call written out as an array (monoStaticSensing.m:1 returns echoGrid; cellSimulation.m:194-197 only ever hands it to fft2D, which is
// why the fused call may keep it as a descriptor): the un-fused synthesis kernel on the descriptor's own inputs -- the same expression, the same bits as the fused kernel's
// store would have been -- or a copy of the context-owned buffer.  d_echo_grid [n_sc x L_out x A].
extern "C" int isac_echo_grid_materialize_dev(isac_ctx* ctx, isac_c64* d_echo_grid, int32_t* dims3) {
  ISAC_ENTER(ctx);
  const LazyEcho& lz = ctx->lazy;
  if (!lz.valid) return fail(ctx, ISAC_ERR_INVALID_ARG, "no lazy echo grid on this context (isac_mono_static_sensing_fused_dev with d_echo_grid == NULL comes first)");
  if (dims3) { dims3[0] = lz.K; dims3[1] = lz.L_out; dims3[2] = lz.A; }
  if (!d_echo_grid) return ISAC_OK;                                  // size query
  const size_t bytes = sizeof(c64) * (size_t)lz.K * lz.L_out * lz.A;
  if (!lz.native) {
    ISAC_HIP(hipMemcpyAsync(d_echo_grid, ctx->echo_own.p, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return ISAC_OK;
  }
  if (lz.L_out > lz.L_whole) ISAC_HIP(hipMemsetAsync(d_echo_grid, 0, bytes, ctx->stream));
  OfdmGeom g{4096, lz.K, 0, 0, 0};
  return echo_dispatch<1>(lz.Q, [&](auto qc) {     // a native lazy grid has one or two LoS targets
    return launch_echo_spectral<(decltype(qc)::value == 1 ? 1 : 2)>(ctx, g, lz.A, lz.L_whole, lz.L_out, lz.Q, ISAC_NOISE_PHILOX_SPECTRAL, nullptr, lz.sig, lz.seed, (c64*)d_echo_grid);
  });
}

extern "C" int isac_ofdm_demodulate_dev(isac_ctx* ctx, const isac_c64* d_wave, int64_t T, int32_t A,
                                        const isac_carrier* carrier, isac_c64* d_grid, int32_t L) {
  ISAC_ENTER(ctx);
  ISAC_TRY(check_carrier(ctx, carrier));
  if (!d_wave || !d_grid || A <= 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "bad arguments");
  OfdmGeom g = geom_of(carrier);
  const int L_whole = whole_symbols(g, T);
  if (L_whole <= 0) return fail(ctx, ISAC_ERR_SHORT_WAVEFORM, "waveform shorter than one OFDM symbol");
  if (L < L_whole) return fail(ctx, ISAC_ERR_CAPACITY, "grid has fewer symbol columns than the waveform holds");
  ctx->range_cache.touch(d_grid, sizeof(c64) * (size_t)g.n_sc * L * A);   // a cached grid overwritten here drops the cached range rows
  if (L > L_whole) ISAC_HIP(hipMemsetAsync(d_grid, 0, sizeof(c64) * (size_t)g.n_sc * L * A, ctx->stream));
  const c64* tw = nullptr;
  ISAC_TRY(isac_get_twiddles(ctx, g.nfft, &tw));
  ISAC_FFT_DISPATCH(g.nfft, ISAC_TRY((launch_demod<FFT, false>(ctx, g, T, A, L_whole, L, tw, 0, 0, nullptr, 0.0, 0,
                                                               (const c64*)d_wave, (c64*)d_grid))));
  return ISAC_OK;
}

template <class FFT>
static int launch_mod(isac_ctx* ctx, const OfdmGeom& g, const ModIo& io, int A, int L, const c64* tw, const c64* grid,
                      double scale, c64* wave, c64* head, const double* rise) {
  size_t lds = sizeof(c64) * FFT::LDS_ELEMS;
  auto kern = mod_kernel<FFT>;
  ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(kern), lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)(L * A)) /* one column per workgroup */, dim3(256), lds, ctx->stream, g, io, A, L, tw, grid, scale, wave, head, rise);
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}

// modulate L symbols (first symbol `sym0` of its subframe) of grid columns [l_off, l_off + L) into wave rows [t_off, ...)
static int modulate_into(isac_ctx* ctx, const isac_carrier* carrier, const c64* d_grid, int grid_cols, int l_off, int L, int A, int sym0,
                         double amplitude, int n_win, c64* d_wave, long long wave_rows, long long t_off) {
  OfdmGeom g = geom_of(carrier);
  if (n_win < 0 || n_win > g.cp_base) return fail(ctx, ISAC_ERR_INVALID_ARG, "windowing must lie in 0..(short cyclic prefix length)");
  const c64* tw = nullptr;
  ISAC_TRY(isac_get_twiddles(ctx, g.nfft, &tw));
  ModIo io{wave_rows, t_off, grid_cols, l_off, sym0, n_win};
  c64* head = nullptr;
  const double* rise = nullptr;
  if (n_win > 0) {
    ISAC_TRY(ensure(ctx, ctx->stage_c, sizeof(c64) * (size_t)n_win * L * A));
    head = (c64*)ctx->stage_c.p;
    ISAC_TRY(isac_get_rise_window(ctx, n_win, &rise));
  }
  ISAC_FFT_DISPATCH(g.nfft, ISAC_TRY((launch_mod<FFT>(ctx, g, io, A, L, tw, d_grid, amplitude / g.nfft, d_wave, head, rise))));
  if (n_win > 0) {
    hipLaunchKernelGGL(mod_window_kernel, dim3(cdiv((long long)n_win * L * A, 256)), dim3(256), 0, ctx->stream, g, io, A, L, (const c64*)head, rise, d_wave);
    ISAC_HIP(hipGetLastError());
  }
  return ISAC_OK;
}

extern "C" int isac_ofdm_modulate_dev(isac_ctx* ctx, const isac_c64* d_grid, int32_t L, int32_t A,
                                      const isac_carrier* carrier, double amplitude, isac_c64* d_wave, int64_t T) {
  return isac_ofdm_modulate_windowed_dev(ctx, d_grid, L, A, carrier, amplitude, 0, 0, d_wave, T);
}

extern "C" int isac_ofdm_modulate_windowed_dev(isac_ctx* ctx, const isac_c64* d_grid, int32_t L, int32_t A, const isac_carrier* carrier,
                                               double amplitude, int32_t n_slot, int32_t windowing, isac_c64* d_wave, int64_t T) {
  ISAC_ENTER(ctx);
  ISAC_TRY(check_carrier(ctx, carrier));
  if (!d_wave || !d_grid || A <= 0 || L <= 0 || n_slot < 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "bad arguments");
  OfdmGeom g = geom_of(carrier);
  const int sym0 = (n_slot % (carrier->scs_khz / 15)) * 14;           // first symbol of the slot inside its subframe (carrier.NSlot)
  const long long need = symbol_start(sym0 + L, g.nfft, g.cp_base, g.cp_long, g.sym_per_half) - symbol_start(sym0, g.nfft, g.cp_base, g.cp_long, g.sym_per_half);
  if (T < need) return fail(ctx, ISAC_ERR_CAPACITY, "waveform buffer shorter than L symbols");
  ctx->range_cache.touch(d_wave, sizeof(c64) * (size_t)T * A);
  if (T > need) ISAC_HIP(hipMemsetAsync(d_wave, 0, sizeof(c64) * (size_t)T * A, ctx->stream));
  return modulate_into(ctx, carrier, (const c64*)d_grid, L, 0, L, A, sym0, amplitude, windowing, (c64*)d_wave, T, 0);
}

// gNBPhy.phyTx's senTxGrid / senTxWave accumulation (gNBPhy.m:591-612) for one slot that carried PDSCH.
extern "C" int isac_sentx_append_dev(isac_ctx* ctx, const isac_carrier* carrier, int32_t A, int32_t curr_slot, int32_t is_dl_slot,
                                     const isac_c64* d_slot_grid, double signal_amp, int32_t windowing, isac_c64* d_sen_grid,
                                     int32_t grid_cols, int32_t l_off, isac_c64* d_sen_wave, int64_t wave_rows, int64_t t_off,
                                     int64_t* t_len) {
  ISAC_ENTER(ctx);
  ISAC_TRY(check_carrier(ctx, carrier));
  if (!d_sen_grid || !d_sen_wave || A <= 0 || curr_slot < 0 || l_off < 0 || t_off < 0 || (is_dl_slot && !d_slot_grid))
    return fail(ctx, ISAC_ERR_INVALID_ARG, "bad arguments");
  OfdmGeom g = geom_of(carrier);
  const int L = 14;
  const int sym0 = (curr_slot % (carrier->scs_khz / 15)) * L;
  const long long need = symbol_start(sym0 + L, g.nfft, g.cp_base, g.cp_long, g.sym_per_half) - symbol_start(sym0, g.nfft, g.cp_base, g.cp_long, g.sym_per_half);
  if (t_len) *t_len = need;
  if (l_off + L > grid_cols || t_off + need > wave_rows) return fail(ctx, ISAC_ERR_CAPACITY, "senTxGrid / senTxWave capacity exceeded");
  ctx->range_cache.valid = false;
  const long long n = (long long)g.n_sc * L * A;
  // 'D' slot: the slot's grid (unscaled) and its waveform x signalAmp (:605-608); any other slot type: zeros of the same size (:609-612)
  hipLaunchKernelGGL(copy_slot_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, is_dl_slot ? (const c64*)d_slot_grid : nullptr,
                     (c64*)d_sen_grid, g.n_sc, L, A, grid_cols, l_off);
  ISAC_HIP(hipGetLastError());
  if (is_dl_slot)
    return modulate_into(ctx, carrier, (const c64*)d_slot_grid, L, 0, L, A, sym0, signal_amp, windowing, (c64*)d_sen_wave, wave_rows, t_off);
  ISAC_HIP(hipMemset2DAsync((c64*)d_sen_wave + t_off, sizeof(c64) * (size_t)wave_rows, 0, sizeof(c64) * (size_t)need, (size_t)A, ctx->stream));
  return ISAC_OK;
}

extern "C" int isac_synth_qpsk_grid_dev(isac_ctx* ctx, isac_c64* d_grid, int32_t K, int32_t L, int32_t A, uint64_t seed,
                                        int32_t zero_s_slots) {
  ISAC_ENTER(ctx);
  if (!d_grid || K <= 0 || L <= 0 || A <= 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "bad arguments");
  long long n = (long long)K * L * A;
  ctx->range_cache.touch(d_grid, sizeof(c64) * (size_t)n);
  hipLaunchKernelGGL(synth_qpsk_kernel, dim3(cdiv(n, 256)), dim3(256), 0, ctx->stream, (c64*)d_grid, K, L, A, seed,
                     zero_s_slots);
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}
