// The UPA steering element both 2-D scans form (doa2d.hip: doa2d_scan_kernel; targets.hip: target_scan2d_kernel), in ONE place so that the two cannot drift apart.
#pragma once
#include "isac_common.hpp"

namespace isac {

constexpr double kUpaSpacing = 0.5;   // element spacing / wavelength (music.m:12)

// a_j[r] of scan point j = e + eS az (column-major like the reference's P(e, a)) and element r = n + nH m (music.m:44-55), from the context's table
// tab = [sind(ele) eS | cosd(azi) aS | sind(azi) aS] (get_doa2d_tables, doa.hip).  The phase in one association for every point:
//     arg = ((-2 pi) sind(th)) * fma(m d, cosd(ph), (n d) sind(ph))
// so that mirror twins (ph -+ 180, -th) -- whose table entries are exact negatives -- get bitwise equal elements.
__device__ __forceinline__ c64 upa_steer(const double* __restrict__ tab, int eS, int aS, int nH, int j, int r) {
  const double* sth = tab;
  const double* cph = tab + eS;
  const double* sph = tab + eS + aS;
  const int e = j % eS, az = j / eS;
  const int n = r % nH, m = r / nH;
  const double inner = ::fma((double)m * kUpaSpacing, cph[az], ((double)n * kUpaSpacing) * sph[az]);
  const double arg = ((-2.0 * M_PI) * sth[e]) * inner;
  double s, c;
  sincos(arg, &s, &c);
  return mk(c, s);
}

}  // namespace isac
