// Stand-alone check of csrc/cpi_post.hpp (no HIP, no library): the clipped row span, the merge rule and the scratch carver that the calls on the last completed fft2D
// share, each against a restatement written out here from the definitions -- include/isac_clean.h steps 7 and 8, include/isac_refine.h step 4.
// Built and run by tests/test_cpi_post_cpu.py; exit status 0 = every check held.
#include <climits>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "cpi_post.hpp"

namespace {

int failures = 0;

void fail_line(const char* what, long long a, long long b, long long c, long long got, long long want) {
  if (++failures <= 20) std::fprintf(stderr, "%s (%lld, %lld, %lld): got %lld, expected %lld\n", what, a, b, c, got, want);
}

// step 8: the rows r of 0 .. nr - 1 with |r - wr| <= span_rows, found by looking at every row
long long check_spans() {
  long long n = 0;
  for (int nr = 1; nr <= 40; ++nr)
    for (int wr = 0; wr < nr; ++wr)
      for (int span_rows : {0, 1, 2, nr, INT_MAX}) {
        int lo = -1, hi = -1;
        for (int r = 0; r < nr; ++r) {
          const long long dist = r > wr ? (long long)r - wr : (long long)wr - r;
          if (dist > span_rows) continue;
          if (lo < 0) lo = r;
          hi = r;
        }
        const isac::RowSpan s = isac::span_of(wr, span_rows, nr);
        if (s.lo != lo) fail_line("span_of lo", wr, span_rows, nr, s.lo, lo);
        if (s.hi != hi) fail_line("span_of hi", wr, span_rows, nr, s.hi, hi);
        if (s.len() != hi - lo + 1) fail_line("span_of len", wr, span_rows, nr, s.len(), hi - lo + 1);
        ++n;
      }
  return n;
}

// a small generator of its own: the lists must be the same on every run and every host
struct Lcg {
  uint64_t s;
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
  int below(int n) { return (int)(next() % (uint32_t)n); }
};

// step 7 as the header states it: "parent[i] = the FIRST earlier kept entry k (parent[k] == k) with |r - row[k]| <= span_rows and |nu[i] - nu[k]| L <= merge_tol ...
// Otherwise parent[i] = i (kept).  merge_tol == 0 disables the step."  With a status array (step 4 of isac_refine.h): only entries with status 0 merge or absorb.
int parent_restated(int i, const std::vector<int32_t>& row, const std::vector<double>& nu, const std::vector<int32_t>& parent, const int32_t* status, int rows, double tol, int L) {
  if (tol == 0.0) return i;
  if (status && status[i] != 0) return i;
  int found = -1;
  for (int k = i - 1; k >= 0; --k) {                                      // descending: the last one seen is the first in input order
    const bool kept = parent[(size_t)k] == k && (!status || status[k] == 0);
    const long long dr = (long long)row[(size_t)i] - row[(size_t)k];
    const double dnu = nu[(size_t)i] > nu[(size_t)k] ? nu[(size_t)i] - nu[(size_t)k] : nu[(size_t)k] - nu[(size_t)i];
    if (kept && (dr < 0 ? -dr : dr) <= rows && dnu * L <= tol) found = k;
  }
  return found < 0 ? i : found;
}

long long check_merges() {
  Lcg g{20240607};
  const double tols[] = {0.0, 0.25, 0.5, 1.0};
  long long n_lists = 0, n_merged = 0, n_equal_nu = 0;
  for (int list = 0; list < 400; ++list) {
    const int n = 1 + g.below(12), L = 4 + g.below(60), rows = g.below(4);
    const double tol = tols[list % 4];
    const bool with_status = list % 3 == 0;
    std::vector<int32_t> row((size_t)n), status((size_t)n), parent((size_t)n), want((size_t)n);
    std::vector<double> nu((size_t)n);
    for (int i = 0; i < n; ++i) {
      row[(size_t)i] = 10 + g.below(6);
      nu[(size_t)i] = (g.below(9) - 4) * 0.25 / L + (g.below(3) == 0 ? 0.0 : g.below(100) * 1e-3 / L);   // a coarse grid of tones: equal nu are common
      status[(size_t)i] = g.below(5) == 0 ? 1 : 0;
      if (i > 0 && g.below(4) == 0) { nu[(size_t)i] = nu[(size_t)g.below(i)]; ++n_equal_nu; }
    }
    const int32_t* st = with_status ? status.data() : nullptr;
    for (int i = 0; i < n; ++i) {                                          // the callers' loops: entry after entry, the earlier parents final
      want[(size_t)i] = parent_restated(i, row, nu, want, st, rows, tol, L);
      parent[(size_t)i] = st && st[i] != 0 ? i : isac::merge_parent(i, row.data(), nu.data(), parent.data(), st, rows, tol, L);
      if (parent[(size_t)i] != want[(size_t)i]) fail_line("merge_parent", list, i, n, parent[(size_t)i], want[(size_t)i]);
      if (tol == 0.0 && parent[(size_t)i] != i) fail_line("merge_tol = 0 merged", list, i, n, parent[(size_t)i], i);
      n_merged += parent[(size_t)i] != i;
    }
    ++n_lists;
  }
  if (n_merged < 100) fail_line("too few merges for the test to mean anything", 0, 0, 0, n_merged, 100);
  if (n_equal_nu < 100) fail_line("too few equal nu", 0, 0, 0, n_equal_nu, 100);
  return n_lists;
}

long long check_carver() {
  Lcg g{77};
  long long n = 0;
  for (int block = 0; block < 200; ++block) {
    isac::Carver cv;
    if (cv.total != 0) fail_line("carver: an empty block", block, 0, 0, (long long)cv.total, 0);
    size_t end_prev = 0, off_last = 0, bytes_last = 0;
    const int regions = 1 + g.below(10);
    for (int r = 0; r < regions; ++r) {
      const size_t bytes = g.below(5) == 0 ? 0 : (size_t)g.below(4) * 16 + (size_t)g.below(3) * (size_t)g.below(40);
      const size_t off = cv.take(bytes);
      if (off % 16 != 0) fail_line("carver: alignment", block, r, (long long)bytes, (long long)off, 0);
      if (off < end_prev) fail_line("carver: overlap", block, r, (long long)bytes, (long long)off, (long long)end_prev);
      if (off >= end_prev + 16) fail_line("carver: a gap of 16 bytes or more", block, r, (long long)bytes, (long long)off, (long long)end_prev);
      if (end_prev % 16 == 0 && off != end_prev) fail_line("carver: regions of 16-byte multiples are adjacent", block, r, (long long)bytes, (long long)off, (long long)end_prev);
      end_prev = off + bytes; off_last = off; bytes_last = bytes;
      ++n;
    }
    if (cv.total != off_last + bytes_last) fail_line("carver: total", block, regions, 0, (long long)cv.total, (long long)(off_last + bytes_last));
  }
  return n;
}

}  // namespace

int main() {
  const long long n_span = check_spans(), n_lists = check_merges(), n_regions = check_carver();
  if (failures) { std::fprintf(stderr, "%d checks failed\n", failures); return 1; }
  std::printf("%lld spans, %lld entry lists, %lld regions OK\n", n_span, n_lists, n_regions);
  return 0;
}
