// Host check of csrc/beam_stream.hpp: the unit-to-thread schedule of cov_noise_beam_kernel (cov.hip).  Plain C++, its own main, no HIP and no library.
// For every shape it walks each workgroup the way the kernel does -- the slab steps with their cursors (unit n of the workgroup's table, step i of the unit), then the
// tail loop -- and counts the loads of every (unit, antenna); a unit's 256 threads hold its 256 samples, one each, so that count is the count of every
// (unit, sample, antenna).  Required: exactly one load each, every unit started inside the stream also stored there, no load in a workgroup's last step.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "beam_stream.hpp"

using namespace isac;

static long long checks = 0;
#define REQUIRE(c)                                                             \
  do {                                                                         \
    ++checks;                                                                  \
    if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } \
  } while (0)

// cov.hip: slabs per symbol column and the staged grid (restated)
static int s_col(int K) {
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

static void walk(int K, int L, int A, long long d) {
  const Numerology nu = numerology(4096, 30);
  const long long T = symbol_start(L, nu.nfft, nu.cp_base, nu.cp_long, nu.sym_per_half);
  const BeamWindow bw = beam_window(nu.nfft, nu.cp_base, nu.cp_long, nu.sym_per_half, L, T, d, d);
  const long long n_units = bw_units(bw), n_slabs = (long long)L * s_col(K);
  long long gx, per;
  staged_grid(n_slabs, gx, per);
  const int spu = bs_steps_per_unit(A);
  REQUIRE(spu * kBeamStreamLoads >= A && (spu - 1) * kBeamStreamLoads < A);
  std::vector<int> count((size_t)n_units * A, 0);
  long long in_stream = 0;
  for (int wg = 0; wg < (int)gx; ++wg) {
    const long long steps = bs_steps_of(n_slabs, per, wg);
    REQUIRE(steps >= 2 && steps % 2 == 0);
    const int mine = bs_units_of(n_units, (int)gx, wg);
    const int n_stream = bs_stream_units(mine, steps, spu);
    REQUIRE(n_stream <= mine && n_stream < kBeamStreamTab);
    int n = 0, i = 0, stored = 0;
    bool fin = false;
    int fin_unit = -1;
    for (long long s = 0; s < steps; ++s) {
      if (fin && fin_unit >= 0) { ++stored; }                                // the fold + store of the unit whose last loads flew during the step before
      const bool active = n < n_stream;
      if (active) {
        REQUIRE(s < steps - 1);                                              // nothing is loaded in the last step: nobody would fold it
        for (int j = 0; j < kBeamStreamLoads; ++j) {
          const int a = bs_antenna(i, j);
          if (a < A) ++count[(size_t)bs_unit((int)gx, wg, n) * A + a];
        }
      }
      const bool last = i == spu - 1;
      fin = last;
      fin_unit = last && active ? n : -1;
      i = last ? 0 : i + 1;
      if (last && n < kBeamStreamTab - 1) ++n;
    }
    REQUIRE(stored == n_stream);
    in_stream += n_stream;
    for (int t = n_stream; t < mine; ++t)
      for (int a = 0; a < A; ++a) ++count[(size_t)bs_unit((int)gx, wg, t) * A + a];
  }
  for (size_t e = 0; e < count.size(); ++e) REQUIRE(count[e] == 1);
  std::printf("K %4d L %3d A %2d: %lld units on %lld workgroups x %lld steps, %lld summed beside the slabs, %lld by the tail loop\n", K, L, A, n_units, gx, per, in_stream,
              n_units - in_stream);
}

int main() {
  const int shapes[][2] = {{288, 14}, {1272, 14}, {3276, 14}, {3276, 28}, {3276, 224}};
  for (const auto& s : shapes)
    for (int A : {49, 56, 64})
      for (long long d : {0ll, 86ll, 390ll}) walk(s[0], s[1], A, d);
  std::printf("beam_stream: %lld checks OK\n", checks);
  return 0;
}
