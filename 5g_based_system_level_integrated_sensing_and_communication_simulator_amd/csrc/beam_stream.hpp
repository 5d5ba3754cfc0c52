// How cov_noise_beam_kernel (cov.hip) spreads the beam-sum's loads over its slab steps: plain C++, host + device (tests/beam_stream_host.cpp walks it with the host
// compiler alone).
//
// The kernel's workgroups walk the units of a BeamWindow (beam_window.hpp: unit = 256 transmit samples of one symbol's range, one sample per thread) grid-stride: workgroup w
// of n_wg owns the units w, w + n_wg, ...  Beside every slab step of its covariance stream a workgroup issues kBeamStreamLoads antenna loads of its running unit -- step i of a
// unit loads the antennas 6 i .. 6 i + 5 (slots at or beyond A load nothing that is summed: the steering image is zero there) -- and folds them one step later, so a unit takes
// bs_steps_per_unit(A) steps and its sums are stored in the step behind its last loads.  Only units that finish inside the stream start there:
//     bs_stream_units = min(units of the workgroup, (steps - 1) / steps_per_unit, kBeamStreamTab - 1)
// (the last step issues no load, the unit table of a workgroup has kBeamStreamTab entries and its last one stays idle); the others are summed by a plain loop behind the last
// slab.  Every (unit, sample, antenna) is therefore loaded exactly once, whichever side runs out first.
#pragma once

#include "beam_window.hpp"

namespace isac {

constexpr int kBeamStreamLoads = 6;   // antenna loads per thread and slab step: 7 units x 11 steps fit the 84 steps of a workgroup at the bench shape (the full slabs: noise_walk.hpp), 12.6 MB in flight device-wide
constexpr int kBeamStreamTab = 32;    // unit table entries per workgroup (LDS)

ISAC_HD inline int bs_steps_per_unit(int A) { return (A + kBeamStreamLoads - 1) / kBeamStreamLoads; }
// units of workgroup wg (grid-stride over n_units)
ISAC_HD inline int bs_units_of(long long n_units, int n_wg, int wg) { return wg < n_units ? (int)((n_units - wg + n_wg - 1) / n_wg) : 0; }
// t-th unit of workgroup wg
ISAC_HD inline long long bs_unit(int n_wg, int wg, int t) { return (long long)wg + (long long)t * n_wg; }
// slab steps workgroup wg runs: its share of n_slabs in chunks of `per` (even), walked in pairs
ISAC_HD inline long long bs_steps_of(long long n_slabs, long long per, int wg) {
  const long long b = (long long)wg * per;
  long long e = b + per;
  if (e > n_slabs) e = n_slabs;
  return e > b ? ((e - b + 1) & ~1ll) : 0;
}
ISAC_HD inline int bs_stream_units(int my_units, long long steps, int steps_per_unit) {
  long long fit = steps > 0 ? (steps - 1) / steps_per_unit : 0;
  if (fit > kBeamStreamTab - 1) fit = kBeamStreamTab - 1;
  return fit < my_units ? (int)fit : my_units;
}
// antenna of load slot j of step i of a unit; >= A: a padding slot
ISAC_HD inline int bs_antenna(int i, int j) { return i * kBeamStreamLoads + j; }

}  // namespace isac
