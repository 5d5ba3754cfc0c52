// The evaluation refine_kernel (refine.hip), clean_cancel_kernel (clean.hip) and the two kernels of relax.hip share: X_a(nu) = sum_l y[l, a] e^{-2 pi j nu l} of one range
// row for every antenna, with the phasors of nu in LDS.  In ONE place so that the tone a cancellation fits is the sum the refinement maximised, bit for bit.  And what a
// cancellation does with it: the phasors that are zero at the inactive symbols (tone_phasors), the least-squares fit and its subtraction from the row (tone_fit_subtract).
#pragma once
#include "isac_common.hpp"

namespace isac {

struct RefineSums { double p, d; };                                        // sum_a |X_a|^2, sum_a Im(conj(X_a) D_a)

__device__ __forceinline__ c64 refine_phasor(double nu, int l) {           // e^{-2 pi j nu l}: sincos of the full argument
  double s, co;
  sincos(((-2.0 * M_PI) * nu) * (double)l, &s, &co);
  return mk(co, s);
}

// (P nFFT, P' nFFT / 4 pi) at the nu whose phasors are s_ph [L]; on return every thread holds the same sums and s_x [A] = X_a(nu).  Ends with a barrier: s_ph, s_p, s_d may
// be rewritten right away.
// AddBack (relax.hip): the sample is y[l, a] + c_back[a] conj(s_back[l]) -- the row with one subtracted tone restored, formed on the fly and never written back; c_back [A]
// (LDS or device memory) holds the tone's amplitudes on this row, s_back [L] (LDS) its phasors, zero at the inactive symbols.  The plain instantiation is the code that
// stood here before the parameter existed: refine_kernel and clean_cancel_kernel keep their bits.
template <bool AddBack = false>
__device__ __forceinline__ RefineSums refine_eval(const c64* __restrict__ row /* ymid + window row */, long long n_rows, int L, int A, const c64* s_ph, c64* s_x, double* s_p,
                                                  double* s_d, const c64* s_back = nullptr, const c64* c_back = nullptr) {
  const int tid = threadIdx.x;
  const int chunk = (L + 3) / 4;
  for (int base = 0; base < 4 * A; base += 256) {                         // (256 = 64 quads: a quad is inside one wave and all of it active or none)
    const int a = (base + tid) >> 2, part = tid & 3;
    c64 x = mk(0.0, 0.0), dx = mk(0.0, 0.0);
    if (a < A) {
      const c64* y = row + n_rows * L * a;
      const int l0 = part * chunk, l1 = min(l0 + chunk, L);
      c64 cb = mk(0.0, 0.0);
      if constexpr (AddBack) cb = c_back[a];
      for (int l = l0; l < l1; ++l) {
        c64 v = y[n_rows * l];
        if constexpr (AddBack) v = v + cb * conj(s_back[l]);
        const c64 z = v * s_ph[l];
        x += z;
        dx = mk(::fma((double)l, z.re, dx.re), ::fma((double)l, z.im, dx.im));
      }
    }
    x.re += __shfl_xor(x.re, 1); x.im += __shfl_xor(x.im, 1); dx.re += __shfl_xor(dx.re, 1); dx.im += __shfl_xor(dx.im, 1);
    x.re += __shfl_xor(x.re, 2); x.im += __shfl_xor(x.im, 2); dx.re += __shfl_xor(dx.re, 2); dx.im += __shfl_xor(dx.im, 2);
    if (a < A && part == 0) {
      s_x[a] = x;
      s_p[a] = x.re * x.re + x.im * x.im;
      s_d[a] = x.re * dx.im - x.im * dx.re;
    }
  }
  __syncthreads();
  RefineSums r{0.0, 0.0};
  for (int a = 0; a < A; ++a) { r.p += s_p[a]; r.d += s_d[a]; }           // ascending antenna order from 0.0; every lane the same address: broadcasts
  __syncthreads();
  return r;
}

// p_nu [L] into s (LDS): e^{-2 pi j nu l}, one sincos of the full argument each, 0 where the symbol is inactive -- a sum over all symbols is then the sum over the active
// ones.  The caller places the barrier.
__device__ __forceinline__ void tone_phasors(c64* s, double nu, int L, const unsigned char* __restrict__ active) {
  for (int l = threadIdx.x; l < L; l += 256) s[l] = active[l] ? refine_phasor(nu, l) : mk(0.0, 0.0);
}

// Step 8 of include/isac_clean.h on one row, by one workgroup of 256 threads: refine_eval<AddBack> with the masked phasors s_ph leaves s_x[a] = X_a summed over the active
// symbols; thread i then rewrites sample (l, a) = (i % L, i / L) of the row, read and written at stride nr, the inactive symbols untouched:
//   plain    y - c conj(p),                               c = X_a / n_active
//   AddBack  (y + C conj(p_old)) - c_new conj(p_new),     C = c_back[a], p_old = s_back: the tone this row held is restored, fitted anew and subtracted in one pass
// s_x stays valid on return (relax_refit_kernel stores the new C from it); no barrier behind the subtraction.
template <bool AddBack>
__device__ __forceinline__ void tone_fit_subtract(c64* row, int nr, int L, int A, const unsigned char* __restrict__ active, double n_active, const c64* s_ph, c64* s_x,
                                                  double* s_p, double* s_d, const c64* s_back = nullptr, const c64* c_back = nullptr) {
  (void)refine_eval<AddBack>(row, nr, L, A, s_ph, s_x, s_p, s_d, s_back, c_back);   // ends with a barrier: every read of the row is done
  for (int i = threadIdx.x; i < L * A; i += 256) {
    const int l = i % L, a = i / L;
    if (!active[l]) continue;
    const c64 c = mk(s_x[a].re / n_active, s_x[a].im / n_active);
    c64* y = row + (long long)nr * (l + (long long)L * a);
    if constexpr (AddBack) *y = (*y + c_back[a] * conj(s_back[l])) - c * conj(s_ph[l]);
    else *y = *y - c * conj(s_ph[l]);
  }
}

}  // namespace isac
