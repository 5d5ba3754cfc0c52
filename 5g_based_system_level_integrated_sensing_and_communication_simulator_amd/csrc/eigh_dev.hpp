// Device-side pieces that the eigensolver (eigh.hip) and MUSIC (music.hip) share: the carve of ctx->eig_scratch and the wavefront reductions.
#pragma once
#include "isac_common.hpp"

namespace isac {

struct EighScratch {   // carve of ctx->eig_scratch for order n
  c64 *M, *Z, *tau, *rot;
  double *d, *e, *scale;
  double* wsc;         // [n] eigenvalues of the (safe-scaled) tridiagonal, ascending -- eigh_bisect_kernel
  char* xch;           // exchange area of eigh_tridiag_dist_kernel (kTdXchBytes, 128-byte aligned)
  int *desc, *cnt;     // desc: (mm, l, first rotation, -) per sweep; cnt: {sweeps published, n_rot, overflow, zungtr done, QL done}
  long long rot_cap;
  int desc_cap;
  __host__ __device__ static size_t bytes(int n) {
    return sizeof(c64) * ((size_t)2 * n * n + n + (size_t)16 * n * n) + sizeof(double) * (3 * n + 4) + sizeof(int) * (4 * (size_t)(30 * n + 2) + 8) + 256 +
           kXchBytes;
  }
  static constexpr size_t kXchBytes = 2048 + 2 * 256 * 64;               // per-wavefront (maximum, XCC id) | 2 parities x 256 rows x (p_i, next column's entry) as tagged granules: at the
                                                                           // START of the scratch, wherever n puts the rest (the host zeroes a fresh allocation)
  __host__ __device__ EighScratch(void* base, int n) {
    xch = reinterpret_cast<char*>(base);
    c64* p = reinterpret_cast<c64*>(xch + kXchBytes);
    M = p; p += (size_t)n * n;
    Z = p; p += (size_t)n * n;
    tau = p; p += n;
    rot = p; rot_cap = (long long)16 * n * n; p += rot_cap;
    d = reinterpret_cast<double*>(p);
    e = d + n;
    scale = e + n + (n & 1);
    desc_cap = 30 * n + 2;
    desc = reinterpret_cast<int*>(scale + 2);       // 16-byte aligned (rot is, and n + (n & 1) + 2 doubles follow)
    cnt = desc + 4 * (size_t)desc_cap;
    wsc = reinterpret_cast<double*>(cnt + 8);       // 16-byte aligned (desc is, 16 desc_cap + 32 bytes follow)
  }
};

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
