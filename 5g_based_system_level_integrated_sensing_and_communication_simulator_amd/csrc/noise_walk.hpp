// The slab walk of the split lazy covariance's noise term (cov.hip): plain C++, host + device (tests/noise_walk_host.cpp enumerates it with the host compiler alone).
//
// A symbol column's K rows are cut into 1024-row blocks; Philox slot 512 b + x (x = 0..511) of block b serves the pair of rows 1024 b + x and 1024 b + 512 + x with its
// outputs 0-1 and 2-3 (echo_dev.hpp).  A slab holds 16 sample slots: 8 consecutive slots x of a block, first halves in sample slots 0..7, second halves in 8..15.
//   * FULL slabs -- at least one second-half row below K -- are walked by cov_noise_beam_kernel, in the order of the regenerating route: every block but the last is
//     complete (64 full slabs), and the full slabs of the last block are its first ones, so full slab sc of a column is slab sc & 63 of block sc >> 6, as before.
//   * HALF slabs -- no second-half row below K -- all lie in the last block, behind its full slabs.  cov_noise_tail_kernel packs them two to a slab: packed slab u holds
//     the first halves of half slab 2 u in sample slots 0..7 and those of half slab 2 u + 1 in sample slots 8..15 (an odd count: the last packed slab's second half is empty).
// Rows at or beyond K stay masked in either walk.
#pragma once

#include "ofdm_symbol.hpp"

namespace isac {

struct NoiseWalk {
  int s_full;    // full slabs per symbol column (cov_noise_beam_kernel)
  int n_half;    // half slabs per symbol column
  int n_packed;  // packed slabs per symbol column (cov_noise_tail_kernel): ceil(n_half / 2)
  int blk;       // the block that holds the half slabs (the column's last)
  int j0;        // its first half slab: slabs j0 .. j0 + n_half - 1 of the block
};

ISAC_HD inline NoiseWalk noise_walk(int K) {
  NoiseWalk w{0, 0, 0, 0, 0};
  if (K <= 0) return w;
  w.blk = (K - 1) >> 10;
  const int rest = K - (w.blk << 10);                             // rows of the last block: 1..1024
  const int first = rest < 512 ? rest : 512, second = rest - first;
  w.j0 = (second + 7) / 8;
  w.s_full = 64 * w.blk + w.j0;
  w.n_half = (first + 7) / 8 - w.j0;
  w.n_packed = (w.n_half + 1) / 2;
  return w;
}
// full slab sc of a column: row of pair row p's first half (second half: + 512) and its Philox slot
ISAC_HD inline int nw_full_row(int sc, int p) { return ((sc >> 6) << 10) + ((sc & 63) << 3) + p; }
ISAC_HD inline int nw_full_slot(int sc, int p) { return ((sc >> 6) << 9) + ((sc & 63) << 3) + p; }
// packed slab u of a column, half h (sample slots 8 h + p): whether it holds a half slab, its rows and Philox slots (outputs 0-1)
ISAC_HD inline bool nw_tail_has(const NoiseWalk& w, int u, int h) { return 2 * u + h < w.n_half; }
ISAC_HD inline int nw_tail_row(const NoiseWalk& w, int u, int h, int p) { return (w.blk << 10) + ((w.j0 + 2 * u + h) << 3) + p; }
ISAC_HD inline int nw_tail_slot(const NoiseWalk& w, int u, int h, int p) { return (w.blk << 9) + ((w.j0 + 2 * u + h) << 3) + p; }

// Workgroups of the tail kernel and packed slabs per workgroup (even: the staged body walks slabs in pairs).  The kernel runs beside the range kernel, off the CPI's
// serial chain, and must be long done when the covariance's reduction wants its partials: at most kNoiseTailSteps steps per workgroup -- a fifth of what a workgroup of
// the main kernel walks at the bench shape (84), so a fifth of its time even where it gets a compute unit's issue slots no faster -- until 512 workgroups are out.
constexpr int kNoiseTailSteps = 16;
ISAC_HD inline void noise_tail_grid(long long slabs, long long& gx, long long& per) {
  per = kNoiseTailSteps;
  if (slabs > 512ll * per) per = ((slabs + 511) / 512 + 1) & ~1ll;
  if (per > slabs) per = (slabs + 1) & ~1ll;
  gx = per > 0 ? (slabs + per - 1) / per : 0;
}

}  // namespace isac
