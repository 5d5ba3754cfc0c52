// csrc/ofdm_symbol.hpp on the host (plain C++, its own main, no HIP, no library): prints what the header computes, for tests/test_numerology_cpu.py to compare with the oracle
// (oracle/ofdm.py: cp_lengths, symbol_starts) -- nothing is checked here, so that the expected values come from the oracle alone.
//   N <nfft> <scs> <mu> <cp_base> <cp_long> <sym_per_half>                         numerology()
//   S <nfft> <scs> <l> <cp> <start> <count(start - 1)> <count(start)> <count(start + 1)>   cp_of_symbol(), symbol_start(), and the whole-symbol count of a waveform of T samples
// by isac_ofdm_symbol_count's rule, the largest L with symbol_start(L) <= T (csrc/echo.hip: whole_symbols), found here by walking L upwards.
// Nfft 128 ... 4096, 15 / 30 / 60 / 120 kHz, symbols 0 ... 2 sym_per_half + 1: past the third long-CP symbol of every numerology.
#include <cstdio>
#include <initializer_list>

#include "ofdm_symbol.hpp"

using namespace isac;

static int count_whole(const Numerology& n, long long T) {
  int L = 0;
  while (symbol_start(L + 1, n.nfft, n.cp_base, n.cp_long, n.sym_per_half) <= T) ++L;
  return L;
}

int main() {
  for (int nfft = 128; nfft <= 4096; nfft *= 2)
    for (int scs : {15, 30, 60, 120}) {
      const Numerology n = numerology(nfft, scs);
      std::printf("N %d %d %d %d %d %d\n", nfft, scs, n.mu, n.cp_base, n.cp_long, n.sym_per_half);
      const int last = 2 * 7 * (scs / 15) + 1;                 // (from the spacing, not from the header's sym_per_half)
      for (int l = 0; l <= last; ++l) {
        const long long s = symbol_start(l, n.nfft, n.cp_base, n.cp_long, n.sym_per_half);
        std::printf("S %d %d %d %d %lld %d %d %d\n", nfft, scs, l, cp_of_symbol(l, n.cp_base, n.cp_long, n.sym_per_half), s, s > 0 ? count_whole(n, s - 1) : 0,
                    count_whole(n, s), count_whole(n, s + 1));
      }
    }
  return 0;
}
