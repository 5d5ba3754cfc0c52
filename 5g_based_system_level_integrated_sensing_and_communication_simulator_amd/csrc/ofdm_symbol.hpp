// OFDM numerology (TS 38.211 5.3.1) and where the CP-OFDM symbols of a waveform start: plain C++, host + device, no HIP header needed
// (tests/beam_window_host.cpp compiles it with the host compiler alone).
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define ISAC_HD __host__ __device__
#else
#define ISAC_HD
#endif

namespace isac {

struct Numerology {
  int nfft, mu, cp_base, cp_long, sym_per_half;  // long CP every sym_per_half symbols
};
inline Numerology numerology(int nfft, int scs_khz) {
  Numerology n{};
  n.nfft = nfft;
  n.mu = 0;
  for (int s = scs_khz / 15; s > 1; s >>= 1) n.mu++;
  double scale = nfft / 2048.0;
  n.cp_base = (int)std::lround(144.0 * scale);
  n.cp_long = n.cp_base + (int)std::lround(16.0 * scale * (1 << n.mu));
  n.sym_per_half = 7 * (1 << n.mu);
  return n;
}
ISAC_HD inline int cp_of_symbol(int l, int cp_base, int cp_long, int sym_per_half) {
  return (l % sym_per_half) == 0 ? cp_long : cp_base;
}
// start sample (of the CP) of symbol l
ISAC_HD inline long long symbol_start(int l, int nfft, int cp_base, int cp_long, int sym_per_half) {
  long long n_long = (l + sym_per_half - 1) / sym_per_half;  // long-CP symbols among 0..l-1
  return (long long)l * (nfft + cp_base) + n_long * (cp_long - cp_base);
}

}  // namespace isac
