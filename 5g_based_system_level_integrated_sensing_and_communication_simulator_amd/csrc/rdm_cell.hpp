// One cell of the range-Doppler map from the range rows: rdm(r, c, a) as a single-bin DFT over the symbols of row r, in ONE place so that the snapshots of the per-target
// lists (targets.hip: target_snapshot) and the complex window of isac_fft2d_get_rdm_window / isac_fft2d_beam_detect (beams.hip: rdm_window_kernel) are the same bits.
// The chain of a cell: the Lu = min(L, nFFT) symbols (fft(., nFFT, 2) truncates) in four quarters of ceil(Lu / 4); quarter p runs acc = fma(y[lsrc], tw[m], acc) over its
// symbols in ascending order from 0, lsrc = the symbol after the half swap (ifftshift), m = li kbin mod nFFT stepped by kbin; the cell is ((q0 + q1) + (q2 + q3)) / sqrt(nFFT).
#pragma once
#include "isac_common.hpp"

namespace isac {

__device__ __forceinline__ int rdm_bin_of_column(int c /* rdm column, 0-based */, int n_fft) { return (c + n_fft / 2) % n_fft; }   // fftshift: column c <-> bin (c + nFFT/2) mod nFFT

// Quarter `part` (0..3) of the chain.  sym: symbol 0 of the cell's row and antenna, the symbols sym_stride elements apart (global memory or LDS).
__device__ __forceinline__ c64 rdm_cell_quarter(const c64* sym, long long sym_stride, int L, int n_fft, int kbin, int part, const c64* __restrict__ tw_d /* e^{-2 pi j m / n_fft} */) {
  const int Lu = L < n_fft ? L : n_fft;
  const int half = L / 2;                                                 // ifftshift over the symbols
  const int chunk = (Lu + 3) / 4;
  const int li0 = part * chunk, li1 = min(li0 + chunk, Lu);
  int m = (int)(((long long)li0 * kbin) % n_fft);
  c64 acc = mk(0.0, 0.0);
  for (int li = li0; li < li1; ++li) {
    int lsrc = li + half;
    if (lsrc >= L) lsrc -= L;
    acc = fma(sym[sym_stride * lsrc], tw_d[m], acc);
    m += kbin;
    if (m >= n_fft) m -= n_fft;
  }
  return acc;
}

// (q0 + q1) + (q2 + q3), then fft(.)/sqrt(nFFT)  fft2D.m:46 -- the order of the two butterfly steps target_snapshot joins its four lanes with
__device__ __forceinline__ c64 rdm_cell_scale(c64 sum, double sqrt_nfft) { return mk(sum.re / sqrt_nfft, sum.im / sqrt_nfft); }
__device__ __forceinline__ c64 rdm_cell_join(c64 q0, c64 q1, c64 q2, c64 q3, double sqrt_nfft) {
  const c64 lo = mk(q0.re + q1.re, q0.im + q1.im), hi = mk(q2.re + q3.re, q2.im + q3.im);
  return rdm_cell_scale(mk(lo.re + hi.re, lo.im + hi.im), sqrt_nfft);
}

}  // namespace isac
