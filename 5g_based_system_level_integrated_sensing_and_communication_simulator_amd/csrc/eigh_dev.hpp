// Device-side pieces that the eigensolver (eigh.hip) and MUSIC (music.hip) share: the pointers into ctx->eig_scratch, the status helpers, zlarfg and the
// wavefront reductions.  The geometry behind them: eigh_layout.hpp.
#pragma once
#include "isac_common.hpp"
#include "eigh_layout.hpp"

namespace isac {

struct EighScratch {   // pointers into ctx->eig_scratch for order n (the carve: EighScratchLayout)
  c64 *M, *Z, *tau, *rot;
  double *d, *e, *scale;
  double* wsc;         // [n] eigenvalues of the (safe-scaled) tridiagonal, ascending -- eigh_bisect_kernel
  char* xch;           // exchange area of eigh_tridiag_dist_kernel
  int *desc, *cnt;     // desc: (mm, l, first rotation, -) per sweep; cnt: {sweeps published, n_rot, overflow, zungtr done, QL done}
  long long rot_cap;
  int desc_cap;
  static constexpr size_t kXchBytes = EighScratchLayout::kXchBytes;
  __host__ __device__ static size_t bytes(int n) { return EighScratchLayout::of(n).bytes; }
  __host__ __device__ EighScratch(void* base, int n) {
    const EighScratchLayout l = EighScratchLayout::of(n);
    char* b = reinterpret_cast<char*>(base);
    xch = b + l.xch;
    M = reinterpret_cast<c64*>(b + l.M); Z = reinterpret_cast<c64*>(b + l.Z); tau = reinterpret_cast<c64*>(b + l.tau); rot = reinterpret_cast<c64*>(b + l.rot);
    d = reinterpret_cast<double*>(b + l.d); e = reinterpret_cast<double*>(b + l.e); scale = reinterpret_cast<double*>(b + l.scale);
    desc = reinterpret_cast<int*>(b + l.desc); cnt = reinterpret_cast<int*>(b + l.cnt); wsc = reinterpret_cast<double*>(b + l.wsc);
    rot_cap = l.rot_cap; desc_cap = l.desc_cap;
  }
};

// The final status of a kernel behind the tridiagonalisation: a timed-out distributed tridiagonalisation stays reported.
__device__ __forceinline__ void eigh_set_status(EighInfo* __restrict__ info, int status) {
  info->status = info->sticky == kEighTridiagTimeout ? kEighTridiagTimeout : status;
}
// eigh_tridiag_dist_kernel gave up (sticky: the kernels behind it overwrite `status`)
__device__ __forceinline__ void eigh_mark_tridiag_timeout(EighInfo* __restrict__ info) { info->status = info->sticky = kEighTridiagTimeout; }

// zlarfg: the reflector of (alpha, x) with |x|^2 = xnorm2 -- beta, tau and scale = 1 / (alpha - beta).  RCP = false: divisions (the one-workgroup kernels);
// RCP = true: two reciprocals instead of four divisions (the distributed kernel).  The two forms round differently and both are pinned: do not unify.
struct Zlarfg { double beta; c64 tau, scale; };
template <bool RCP>
__device__ __forceinline__ Zlarfg zlarfg(const c64 alpha, const double xnorm2) {
  Zlarfg r{alpha.re, mk(0.0, 0.0), mk(0.0, 0.0)};
  if (xnorm2 != 0.0 || alpha.im != 0.0) {
    r.beta = -copysign(sqrt(alpha.re * alpha.re + alpha.im * alpha.im + xnorm2), alpha.re);
    if constexpr (RCP) {
      const double ib = 1.0 / r.beta;
      r.tau = mk((r.beta - alpha.re) * ib, -alpha.im * ib);
      const c64 dlt = mk(alpha.re - r.beta, alpha.im);
      const double idn = 1.0 / (dlt.re * dlt.re + dlt.im * dlt.im);
      r.scale = mk(dlt.re * idn, -dlt.im * idn);
    } else {
      r.tau = mk((r.beta - alpha.re) / r.beta, -alpha.im / r.beta);
      const c64 dlt = mk(alpha.re - r.beta, alpha.im);
      const double dn = dlt.re * dlt.re + dlt.im * dlt.im;
      r.scale = mk(dlt.re / dn, -dlt.im / dn);
    }
  }
  return r;
}

__device__ __forceinline__ double rcp_fast(double q) {   // 1/q: hardware estimate r0 + one third-order step  r0 (1 + h + h^2), h = 1 - q r0
  const double r0 = __builtin_amdgcn_rcp(q);
  const double h = ::fma(-q, r0, 1.0);
  return ::fma(r0, ::fma(h, h, h), r0);
}
__device__ __forceinline__ double wave_sum(double x) { for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o); return x; }
__device__ __forceinline__ double wave_max(double x) { for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o)); return x; }
__device__ __forceinline__ double wave_min(double x) { for (int o = 32; o > 0; o >>= 1) x = fmin(x, __shfl_xor(x, o)); return x; }

// Sum over the 64 lanes of a wavefront through DPP row operations (quad_perm, row_ror, row_bcast15 / 31 + one readlane): six short VALU
// steps.  The __shfl_xor butterfly goes through the LDS crossbar (ds_bpermute: ~100 cycles per step, six dependent steps) -- for the
// one-reduction-per-Householder-step kernels of eigh.hip and music.hip that latency WAS the kernel (two of them per reflector: 37 of the 83 us of the subspace
// kernel at n = 64).  Returns the total in every lane (wave-uniform).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_move(double x) {
  const int lo = __double2loint(x), hi = __double2hiint(x);
  const int l2 = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xf, false);    // rows outside ROW_MASK receive 0: the add leaves them unchanged
  const int h2 = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xf, false);
  return __hiloint2double(h2, l2);
}
__device__ __forceinline__ double wave_sum_dpp(double x) {
  x += dpp_move<0xB1, 0xf>(x);                       // quad_perm [1,0,3,2]
  x += dpp_move<0x4E, 0xf>(x);                       // quad_perm [2,3,0,1]
  x += dpp_move<0x124, 0xf>(x);                      // row_ror:4
  x += dpp_move<0x128, 0xf>(x);                      // row_ror:8   -> every lane: the sum of its row of 16
  x += dpp_move<0x142, 0xa>(x);                      // row_bcast15 -> rows 1, 3 += rows 0, 2
  x += dpp_move<0x143, 0xc>(x);                      // row_bcast31 -> rows 2, 3 += rows 0 + 1: lane 63 holds the total
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), 63), __builtin_amdgcn_readlane(__double2loint(x), 63));
}
}  // namespace isac
