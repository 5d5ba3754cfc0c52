// One cell of a beam plane and of the map over the planes, in ONE place so that isac_fft2d_beam_detect (beams.hip: beam_planes_kernel; targets.hip: target_cells_kernel<true>)
// and the band update of isac_fft2d_beam_clean_targets (beam_clean.hip) form the same bits.  Steps 2 and 4 of include/isac_beams.h:
//   Z = sum_a conj(W[a, b]) Y[a], ascending a from 0 with the fused multiply-adds of fma(c64, c64, c64) -- the callers' loop, kBeamTile accumulators per lane;
//   Pb = (re^2 + im^2) / n_b: two rounded products, one rounded sum, one rounded division -- never contracted;
//   M = the maximum over the planes, b* its first plane in ascending order; a NaN never wins, and M is NaN only where every plane is.
#pragma once
#include "isac_common.hpp"

namespace isac {

constexpr int kBeamTile = 8;                                              // beams per lane: accumulators in registers, their conjugated weights side by side in LDS

__device__ __forceinline__ double beam_cell_power(c64 z, double n_b) { return __ddiv_rn(__dadd_rn(__dmul_rn(z.re, z.re), __dmul_rn(z.im, z.im)), n_b); }

// p: the cell in plane 0, the planes `plane` doubles apart.  Returns M; *best = b*.
__device__ __forceinline__ double planes_first_max(const double* __restrict__ p, long long plane, int n_planes, int* best) {
  double s = __builtin_nan("");
  int arg = 0;
  for (int a = 0; a < n_planes; ++a) {
    const double v = p[plane * a];
    if (v > s || (s != s && v == v)) { s = v; arg = a; }                  // strictly greater: the first maximum stays
  }
  *best = arg;
  return s;
}

}  // namespace isac
