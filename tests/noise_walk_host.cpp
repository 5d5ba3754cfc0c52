// Host check of csrc/noise_walk.hpp: the slab walk of the split lazy covariance's noise term (cov_noise_beam_kernel: the full slabs; cov_noise_tail_kernel: the half slabs,
// packed two to a slab).  Plain C++, its own main, no HIP and no library.
// For every K in 8 .. 4096 it enumerates (slab, sample slot) -> (row, Philox slot, half) of both kernels the way their sources do -- masks included -- and requires: every
// row k < K exactly once, no row >= K, every element's (Philox slot, half) the field's own (row = 1024 (slot div 512) + slot mod 512 + 512 half), the tail kernel on first
// halves only.  Then the step counts: the workgroups of the main kernel walk L x s_full slabs between them, in pairs, and what bs_stream_units is handed are those steps
// (at the bench shape 84 per workgroup for the 77 its 7 beam units need); the tail kernel's grid covers L x n_packed slabs in chunks of at most kNoiseTailSteps until 512
// workgroups are out.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "beam_stream.hpp"
#include "noise_walk.hpp"

using namespace isac;

static long long checks = 0;
#define REQUIRE(c)                                                             \
  do {                                                                         \
    ++checks;                                                                  \
    if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } \
  } while (0)

// cov.hip: slabs per symbol column of the regenerating route and the staged grid (restated)
static int s_col_regenerating(int K) {
  int s = 0;
  for (int k0 = 0; k0 < K; k0 += 1024) s += ((K - k0 < 512 ? K - k0 : 512) + 7) / 8;
  return s;
}
static void staged_grid(long long slabs, long long& gx, long long& per) {
  gx = 512 < slabs ? 512 : slabs;
  per = (slabs + gx - 1) / gx;
  per = (per + 1) & ~1ll;
  gx = (slabs + per - 1) / per;
}

static void element(std::vector<int>& seen, std::vector<int>& slot_seen, int K, int row, int slot, int half) {
  REQUIRE(row >= 0 && row < K);
  REQUIRE(slot >= 0 && slot < 2048);
  REQUIRE(row == ((slot >> 9) << 10) + (slot & 511) + 512 * half);
  ++seen[(size_t)row];
  ++slot_seen[(size_t)(2 * slot + half)];
}

static void column(int K) {
  const NoiseWalk w = noise_walk(K);
  REQUIRE(w.s_full >= 0 && w.n_half >= 0 && w.n_packed == (w.n_half + 1) / 2);
  REQUIRE(w.s_full + w.n_half == s_col_regenerating(K));                     // the same slabs as the regenerating route, cut in two sets
  REQUIRE(w.s_full > 0 || w.n_half > 0);
  std::vector<int> seen((size_t)K, 0), slot_seen(2 * 2048, 0);
  // cov_noise_beam_kernel: full slab sc, pair row p -> sample slots p (first half) and p + 8 (second half); CovNoiseBeamSource::init's masks
  for (int sc = 0; sc < w.s_full; ++sc) {
    int second = 0;
    for (int p = 0; p < 8; ++p) {
      const int k0 = nw_full_row(sc, p), slot = nw_full_slot(sc, p);
      REQUIRE(k0 < K);                                                         // a full slab has no masked first half
      element(seen, slot_seen, K, k0, slot, 0);
      if (k0 + 512 < K) { element(seen, slot_seen, K, k0 + 512, slot, 1); ++second; }
    }
    REQUIRE(second > 0);                                                       // ... and at least one second-half row: it is no half slab
  }
  // cov_noise_tail_kernel: packed slab u, half h, row p -> sample slot 8 h + p; CovNoiseTailSource::init's masks
  int filled = 0;
  for (int u = 0; u < w.n_packed; ++u)
    for (int h = 0; h < 2; ++h) {
      if (!nw_tail_has(w, u, h)) { REQUIRE(h == 1 && u == w.n_packed - 1 && (w.n_half & 1)); continue; }   // an odd count: one empty second half, the last
      ++filled;
      int rows = 0;
      for (int p = 0; p < 8; ++p) {
        const int k = nw_tail_row(w, u, h, p), slot = nw_tail_slot(w, u, h, p);
        REQUIRE(k + 512 >= K);                                                 // no second-half row below K: a half slab
        if (k < K) { element(seen, slot_seen, K, k, slot, 0); ++rows; }
      }
      REQUIRE(rows > 0);
    }
  REQUIRE(filled == w.n_half);
  for (int k = 0; k < K; ++k) REQUIRE(seen[(size_t)k] == 1);
  for (size_t e = 0; e < slot_seen.size(); ++e) REQUIRE(slot_seen[e] <= 1);
}

// the grids of a CPI of L symbols at K subcarriers and what the beam-sum's schedule is handed
static void grids(int K, int L, int A, long long n_units, bool print) {
  const NoiseWalk w = noise_walk(K);
  const long long n_slabs = (long long)L * w.s_full, n_tail = (long long)L * w.n_packed;
  const int spu = bs_steps_per_unit(A);
  long long gx = 0, per = 2, walked = 0, streamed = 0;
  if (n_slabs > 0) {
    staged_grid(n_slabs, gx, per);
    REQUIRE(gx >= 1 && gx <= 512 && per % 2 == 0);
    for (int wg = 0; wg < (int)gx; ++wg) {
      const long long b = (long long)wg * per, e = b + per < n_slabs ? b + per : n_slabs;
      REQUIRE(e > b);
      walked += e - b;
      const long long steps = bs_steps_of(n_slabs, per, wg);
      REQUIRE(steps == ((e - b + 1) & ~1ll));                                  // the steps the staged body runs: its slabs, in pairs
      const int mine = bs_units_of(n_units, (int)gx, wg), n_stream = bs_stream_units(mine, steps, spu);
      REQUIRE(n_stream <= mine && n_stream < kBeamStreamTab && (long long)n_stream * spu <= steps - 1);
      REQUIRE(n_stream == mine || (long long)(n_stream + 1) * spu > steps - 1 || n_stream == kBeamStreamTab - 1);   // as many as fit
      streamed += n_stream;
    }
    REQUIRE(walked == n_slabs);
  } else {
    REQUIRE(bs_steps_of(0, per, 0) == 0 && bs_stream_units(7, 0, spu) == 0);   // no full slab: every unit goes to the loop behind the slabs
  }
  long long gt = 0, per_t = 0;
  if (n_tail > 0) {
    noise_tail_grid(n_tail, gt, per_t);
    REQUIRE(gt >= 1 && gt <= 512 && per_t >= 2 && per_t % 2 == 0);
    REQUIRE(gt * per_t >= n_tail && (gt - 1) * per_t < n_tail);                // every packed slab, no empty workgroup
    REQUIRE(per_t <= kNoiseTailSteps || gt > 448);                             // longer chunks only once the grid is full
  }
  if (print)
    std::printf("K %4d L %3d A %2d: %d full + %d half slabs per column (%d packed); main %lld workgroups x %lld steps, %lld of %lld units beside the slabs; tail %lld x %lld\n", K, L,
                A, w.s_full, w.n_half, w.n_packed, gx, per, streamed, n_units, gt, per_t);
}

int main() {
  for (int K = 8; K <= 4096; ++K) column(K);
  for (int K = 8; K <= 4096; ++K)
    for (int L : {1, 14, 224}) grids(K, L, 64, 16ll * L, false);
  const int shapes[][2] = {{288, 14}, {300, 14}, {624, 14}, {1272, 14}, {3276, 14}, {3276, 224}};
  for (const auto& s : shapes)
    for (int A : {49, 64}) grids(s[0], s[1], A, 16ll * s[1], true);
  {                                                                            // the bench shape: 84 steps per workgroup for the 77 its 7 units need
    const NoiseWalk w = noise_walk(3276);
    REQUIRE(w.s_full == 192 && w.n_half == 26 && w.n_packed == 13);
    long long gx, per;
    staged_grid(224ll * w.s_full, gx, per);
    REQUIRE(gx == 512 && per == 84);
    REQUIRE(bs_stream_units(bs_units_of(3584, 512, 0), bs_steps_of(224ll * w.s_full, per, 0), bs_steps_per_unit(64)) == 7);
  }
  std::printf("noise_walk: %lld checks OK\n", checks);
  return 0;
}
