// csrc/beam_window.hpp on the host (plain C++, its own main, no HIP, no library): which transmit samples the window-walking beam-sum sums, checked by brute force
// against the demodulation windows, which this program lays out by itself (symbol by symbol, adding nfft + cp) rather than through the header's formulas.
//
// Every carrier the library accepts (Nfft 128 ... 4096, 15 / 30 / 60 / 120 kHz), 1 / 2 / 14 / 15 / 29 symbols, a waveform that ends with its last symbol and one with
// 37 samples more (not a multiple of 256), one target at each delay of {0, 1, cp/2 - 1, cp/2, cp/2 + 1, cp, cp + 1, 2 cp} (cp: the normal prefix) and of two longer ones
// (beyond a symbol, beyond 29 symbols), and two targets at every pair of those delays, equal and unequal.
//   1. every (symbol l, n in [0, nfft), target q) with u = w0_l + n - d_q >= 0 has u in exactly one unit;
//   2. every such u < 0 -- the window reads the zero of coef_q[t], t = w0_l + n < d_q, there -- is in exactly one unit as a virtual sample (the kernel writes the zero from it);
//   no sample, needed or not, is in two units, and none lies outside [-d_max, T);
//   3. the samples of [0, T) in a unit number at most L (nfft + d_max - d_min) + 255 units.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "beam_window.hpp"

using namespace isac;

static long long n_checks = 0;

#define REQUIRE(cond, ...)                                       \
  do {                                                           \
    ++n_checks;                                                  \
    if (!(cond)) {                                               \
      std::printf("FAILED %s: ", #cond);                         \
      std::printf(__VA_ARGS__);                                  \
      std::printf("\n");                                         \
      std::exit(1);                                              \
    }                                                            \
  } while (0)

static void check(const Numerology& nu, int scs, int L, long long T, const std::vector<long long>& w0, const std::vector<long long>& d) {
  long long d_min = d[0], d_max = d[0];
  for (long long v : d) { d_min = v < d_min ? v : d_min; d_max = v > d_max ? v : d_max; }
  const BeamWindow bw = beam_window(nu.nfft, nu.cp_base, nu.cp_long, nu.sym_per_half, L, T, d_min, d_max);
  const long long units = bw_units(bw);
  REQUIRE(units >= 1 && bw.units_per_symbol >= 1, "nfft %d scs %d L %d", nu.nfft, scs, L);
  std::vector<unsigned char> hits((size_t)(T + d_max), 0);             // virtual samples [-d_max, T)
  long long real = 0;
  for (long long k = 0; k < units; ++k) {
    const int l = (int)(k / bw.units_per_symbol), j = (int)(k % bw.units_per_symbol);
    const long long lo = bw_first(bw, l), hi = bw_range_end(bw, l);
    for (int i = 0; i < kBeamUnit; ++i) {
      const long long u = bw_sample(bw, l, j, i);
      if (u < lo || u >= hi) continue;
      REQUIRE(u >= -d_max && u < T, "sample %lld outside [-%lld, %lld): nfft %d scs %d L %d", u, d_max, T, nu.nfft, scs, L);
      REQUIRE(hits[(size_t)(u + d_max)] == 0, "sample %lld in two units: nfft %d scs %d L %d d %lld..%lld", u, nu.nfft, scs, L, d_min, d_max);
      hits[(size_t)(u + d_max)] = 1;
      real += u >= 0;
    }
  }
  for (int l = 0; l < L; ++l)
    for (long long dq : d)
      for (int n = 0; n < nu.nfft; ++n) {
        const long long u = w0[(size_t)l] + n - dq;                    // >= 0: the sample coef_q[w0_l + n] is made of (1.); < 0: its zero (2.)
        REQUIRE(u >= -d_max && u < T && hits[(size_t)(u + d_max)] == 1, "symbol %d n %d delay %lld: sample %lld in no unit (nfft %d scs %d L %d T %lld d %lld..%lld)", l, n, dq,
                u, nu.nfft, scs, L, T, d_min, d_max);
      }
  REQUIRE(real <= (long long)L * (nu.nfft + d_max - d_min) + 255 * units, "%lld samples in %lld units: nfft %d scs %d L %d d %lld..%lld", real, units, nu.nfft, scs, L, d_min,
          d_max);
}

int main() {
  long long n_cfg = 0, n_windowed = 0;
  for (int nfft = 128; nfft <= 4096; nfft *= 2)
    for (int scs : {15, 30, 60, 120}) {
      const Numerology nu = numerology(nfft, scs);
      const int cp = nu.cp_base;
      for (int L : {1, 2, 14, 15, 29}) {
        std::vector<long long> w0;                                     // demod_kernel's windows: half a prefix into each symbol, nfft long
        long long at = 0;
        for (int l = 0; l < L; ++l) {
          const int cpl = (l % nu.sym_per_half) == 0 ? nu.cp_long : nu.cp_base;
          w0.push_back(at + cpl / 2);
          at += nfft + cpl;
        }
        const std::vector<long long> delays = {0, 1, cp / 2 - 1, cp / 2, cp / 2 + 1, cp, cp + 1, 2 * cp, 3 * (long long)nfft + 5, 30 * (long long)(nfft + nu.cp_long)};
        for (long long T : {at, at + 37}) {
          for (size_t a = 0; a < delays.size(); ++a) {
            check(nu, scs, L, T, w0, {delays[a]});
            for (size_t b = a; b < delays.size(); ++b) check(nu, scs, L, T, w0, {delays[b], delays[a]});   // (the order of the two does not enter)
            n_cfg += 1 + (long long)(delays.size() - a);
          }
          if (nfft == 4096 && L >= 14) n_windowed += beam_window(nfft, nu.cp_base, nu.cp_long, nu.sym_per_half, L, T, 0, 0).n_sym > 0;
        }
      }
    }
  // the walk over the windows is taken where it has fewer units (where a symbol is shorter than a unit or two, rounding up to whole units eats the prefix): at Nfft = 4096
  // and one delay it saves a unit per symbol
  REQUIRE(n_windowed == 4 * 3 * 2, "%lld", n_windowed);
  std::printf("beam_window: %lld configurations, %lld checks OK\n", n_cfg, n_checks);
  return 0;
}
