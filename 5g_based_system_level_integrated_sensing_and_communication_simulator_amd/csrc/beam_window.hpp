// Which transmit samples the beam-sum in front of the fused spectral route has to sum (beamsum_coef_kernel, echo.hip): plain C++, host + device.
//
// The only reader of coef on that route is the per-target demodulation (demod_kernel<FFT, false>), which reads symbol l's window [w0_l, w0_l + nfft),
// w0_l = symbol_start(l) + cp_l / 2, and coef_q[t] depends on ONE transmit sample, u = t - d_q.  So symbol l needs the samples
//     R_l = [w0_l - d_max, w0_l + nfft - d_min)          (the union over the targets; nfft + d_max - d_min of the symbol's nfft + cp_l samples)
// and nothing of the cyclic prefix in between.  Samples are kept VIRTUAL below zero: u < 0 stands for "before the waveform", whose coef_q[u + d_q] is the zero that the
// window reads there, so one rule covers values and zeros.  R_l and R_{l+1} overlap once d_max - d_min exceeds the gap between two windows; both ends grow with l, so giving
// each symbol only what lies at or beyond the end of its predecessor's range,
//     S_l = [max(w0_l - d_max, end_{l-1}), end_l),       end_l = min(T, w0_l + nfft - d_min),
// leaves every needed sample in exactly one S_l without a table.  A work unit is 256 samples (bw_sample); symbol l owns units_per_symbol = ceil(|R_l| / 256) of them, so
// unit k is (l, j) = (k / units_per_symbol, k % units_per_symbol) -- arithmetic, nothing to upload -- and no unit is empty: at one delay and Nfft = 4096, 16 full units
// per symbol.
// n_sym == 0 is the degenerate walk over every sample, [-d_max, T): what the kernel did before, and what the host picks where it takes fewer units (delays spread wider than
// the cyclic prefix make the ranges tile the whole waveform anyway; no whole symbol cannot occur on that route).
#pragma once

#include "ofdm_symbol.hpp"

namespace isac {

constexpr int kBeamUnit = 256;    // samples per work unit = threads per workgroup
constexpr int kBeamLine = 8;      // samples per 128-byte line

struct BeamWindow {
  int nfft, cp_base, cp_long, sym_per_half;
  int n_sym;               // whole symbols of the waveform; 0: one range over every sample
  int units_per_symbol;
  long long T, d_min, d_max;
};

ISAC_HD inline long long bw_floor_line(long long u) { return u & ~(long long)(kBeamLine - 1); }   // (two's complement: rounds towards minus infinity)
ISAC_HD inline int bw_symbols(const BeamWindow& w) { return w.n_sym > 0 ? w.n_sym : 1; }
ISAC_HD inline long long bw_units(const BeamWindow& w) { return (long long)bw_symbols(w) * w.units_per_symbol; }

// demod_kernel's window start of symbol l
ISAC_HD inline long long bw_window_start(const BeamWindow& w, int l) {
  return symbol_start(l, w.nfft, w.cp_base, w.cp_long, w.sym_per_half) + cp_of_symbol(l, w.cp_base, w.cp_long, w.sym_per_half) / 2;
}
// R_l's start and end_l
ISAC_HD inline long long bw_range_start(const BeamWindow& w, int l) { return (w.n_sym > 0 ? bw_window_start(w, l) : 0) - w.d_max; }
ISAC_HD inline long long bw_range_end(const BeamWindow& w, int l) {
  if (w.n_sym <= 0) return w.T;
  const long long e = bw_window_start(w, l) + w.nfft - w.d_min;
  return e < w.T ? e : w.T;
}
// S_l = [first, end): the samples symbol l's units sum
ISAC_HD inline long long bw_first(const BeamWindow& w, int l) {
  const long long s = bw_range_start(w, l);
  if (l == 0) return s;
  const long long p = bw_range_end(w, l - 1);
  return s > p ? s : p;
}
// sample of thread i of unit j of symbol l; the thread sums it when bw_first <= sample < bw_range_end.  The units start on the line R_l starts in, so that all but
// the first few threads of a symbol load whole lines; those few, in front of R_l, take the samples behind the symbol's last unit instead.
ISAC_HD inline long long bw_sample(const BeamWindow& w, int l, int j, int i) {
  const long long s = bw_range_start(w, l), u = bw_floor_line(s) + (long long)j * kBeamUnit + i;
  return u < s ? u + (long long)w.units_per_symbol * kBeamUnit : u;
}

// Host: the walk for a waveform of T samples with n_sym whole symbols and target delays within [d_min, d_max].
inline BeamWindow beam_window(int nfft, int cp_base, int cp_long, int sym_per_half, int n_sym, long long T, long long d_min, long long d_max) {
  BeamWindow w{nfft, cp_base, cp_long, sym_per_half, n_sym, 0, T, d_min, d_max};
  auto units = [](long long span) { return (span + (kBeamUnit - 1)) / kBeamUnit; };
  const long long per_symbol = units(nfft + (d_max - d_min)), whole = units(T + d_max);
  if (n_sym > 0 && per_symbol * n_sym < whole) {
    w.units_per_symbol = (int)per_symbol;
  } else {
    w.n_sym = 0;
    w.units_per_symbol = whole > 1 ? (int)whole : 1;
  }
  return w;
}

}  // namespace isac
