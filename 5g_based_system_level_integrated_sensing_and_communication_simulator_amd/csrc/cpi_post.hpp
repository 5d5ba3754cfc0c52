// The host arithmetic that the calls on "the last completed fft2D" share (beams.hip, refine.hip, clean.hip, beam_clean.hip, relax.hip): the clipped row span of a
// cancellation, the merge rule of the lists, the layout of a scratch block.  Plain C++, no HIP types: tests/cpi_post_host.cpp checks it on the host.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace isac {

// The window rows wr - span_rows .. wr + span_rows, clipped to 0 .. nr - 1 (0 <= wr < nr, span_rows >= 0; span_rows = 2^31 - 1 does not overflow)
struct RowSpan {
  int lo, hi;
  int len() const { return hi - lo + 1; }
};
inline RowSpan span_of(int wr, int span_rows, int nr) {
  const long long lo = (long long)wr - span_rows, hi = (long long)wr + span_rows;
  return RowSpan{(int)(lo > 0 ? lo : 0), (int)(hi < nr - 1 ? hi : nr - 1)};
}

// Step 7 of include/isac_clean.h (step 4 of include/isac_refine.h with merge_rows): the parent of entry i is the FIRST earlier kept entry k (parent[k] == k) within
// `rows` range rows and merge_tol / L cycles per symbol of it, else i itself.  merge_tol == 0 keeps every entry -- two lobes of one tone can bisect to the very same
// bits, and a tolerance of zero must not depend on that.  status (or NULL: every entry counts): only the entries with status 0 absorb.
inline int merge_parent(int i, const int32_t* row, const double* nu, const int32_t* parent, const int32_t* status, int rows, double merge_tol, int L) {
  if (merge_tol == 0.0) return i;
  for (int k = 0; k < i; ++k)
    if (parent[k] == k && (!status || status[k] == 0) && std::abs(row[i] - row[k]) <= rows && std::fabs(nu[i] - nu[k]) * L <= merge_tol) return k;
  return i;
}

// One scratch block, region after region: take() returns the region's offset, a multiple of 16 bytes; `total` is the size of the block so far.  A region whose size is a
// multiple of 16 has the next one right behind it.
struct Carver {
  size_t total = 0;
  size_t take(size_t bytes) {
    const size_t off = (total + 15) & ~(size_t)15;
    total = off + bytes;
    return off;
  }
};

}  // namespace isac
