// Stand-alone check of csrc/cut_window.hpp (no HIP, no library): every number isac::CutWindow derives from an isac_cfar_config, the CUT ordinal and its inverse,
// and the two estimate formulas, against values written out here by hand from the definitions -- cfar2D.m:17-24 (the CUT rectangle, rows fastest), the
// guard + training halo of phased.CFARDetector2D around it, fft2D.m:77-82 (rngEst = (row - 1) rRes, velEst = (col - nFFT/2 - 1) vRes).
// Built and run by tests/test_cut_window_cpu.py; exit status 0 = every check held.
#include <cstdio>

#include "cut_window.hpp"

namespace {

int failures = 0;

void eq(const char* cfg, const char* what, long long got, long long want) {
  if (got != want) { std::fprintf(stderr, "%s: %s = %lld, expected %lld\n", cfg, what, got, want); ++failures; }
}
void eqd(const char* cfg, const char* what, double got, double want) {
  if (got != want) { std::fprintf(stderr, "%s: %s = %.17g, expected %.17g\n", cfg, what, got, want); ++failures; }
}

struct Geom { int nr, nc, hr, hc, gr, gc, n_cut_rows, n_cut_cols, cap; };   // the fields CutWindow::fill sets, as rdm.hip's CfarGeom / TailGeom name them, and one it does not
struct Cell { int cut, row, col; };                       // CUT ordinal <-> 1-based (row, column) of the map
struct Expect {
  const char* name;
  isac_cfar_config cf;                                    // {pfa, guard, train, row0, row1, col0, col1}
  int gr, gc, hr, hc, n_cut_rows, n_cut_cols, nr, nc, first_row, first_col;
  long long n_cut;
  Cell cells[4];
};

const Expect kCases[] = {
    // the default zone of radarParams: detectionArea 50..500 m x -50..50 m/s at 30 kHz, nIFFT 4096, nFFT 256 -> rows 42..411, columns 118..140; guard [2 2], training [1 1]
    {"default zone", {1e-9, {2, 2}, {1, 1}, 42, 411, 118, 140}, 2, 2, 3, 3, 370, 23, 376, 29, 39, 115, 8510,
     {{0, 42, 118}, {369, 411, 118}, {370, 42, 119}, {8509, 411, 140}}},
    // one cell under test; guard and training differ per dimension
    {"1 x 1 zone", {1e-6, {1, 2}, {2, 1}, 10, 10, 7, 7}, 1, 2, 3, 3, 1, 1, 7, 7, 7, 4, 1,
     {{0, 10, 7}, {0, 10, 7}, {0, 10, 7}, {0, 10, 7}}},
    // no guard band: the halo is the training band alone
    {"guard (0, 0)", {1e-3, {0, 0}, {1, 2}, 5, 8, 20, 22}, 0, 0, 1, 2, 4, 3, 6, 7, 4, 18, 12,
     {{0, 5, 20}, {3, 8, 20}, {4, 5, 21}, {11, 8, 22}}},
    // the first CUT row is hr + 1 (and the first CUT column hc + 1): the window starts at row 1, column 1 of the map
    {"window at the map's first row", {1e-9, {2, 2}, {1, 1}, 4, 9, 4, 4}, 2, 2, 3, 3, 6, 1, 12, 7, 1, 1, 6,
     {{0, 4, 4}, {1, 5, 4}, {4, 8, 4}, {5, 9, 4}}},
};

}  // namespace

int main() {
  for (const Expect& e : kCases) {
    const isac::CutWindow w = isac::CutWindow::of(e.cf);
    eq(e.name, "row0", w.row0, e.cf.row0); eq(e.name, "col0", w.col0, e.cf.col0);
    eq(e.name, "gr", w.gr, e.gr); eq(e.name, "gc", w.gc, e.gc);
    eq(e.name, "hr", w.hr, e.hr); eq(e.name, "hc", w.hc, e.hc);
    eq(e.name, "n_cut_rows", w.n_cut_rows, e.n_cut_rows); eq(e.name, "n_cut_cols", w.n_cut_cols, e.n_cut_cols);
    eq(e.name, "nr", w.nr, e.nr); eq(e.name, "nc", w.nc, e.nc);
    eq(e.name, "first_row", w.first_row, e.first_row); eq(e.name, "first_col", w.first_col, e.first_col);
    eq(e.name, "n_cut", w.n_cut(), e.n_cut);
    Geom g{};                                             // the window part of a kernel's by-value geometry
    w.fill(g);
    eq(e.name, "fill nr", g.nr, e.nr); eq(e.name, "fill nc", g.nc, e.nc); eq(e.name, "fill hr", g.hr, e.hr); eq(e.name, "fill hc", g.hc, e.hc);
    eq(e.name, "fill gr", g.gr, e.gr); eq(e.name, "fill gc", g.gc, e.gc);
    eq(e.name, "fill n_cut_rows", g.n_cut_rows, e.n_cut_rows); eq(e.name, "fill n_cut_cols", g.n_cut_cols, e.n_cut_cols);
    eq(e.name, "fill leaves the rest", g.cap, 0);
    for (const Cell& c : e.cells) {
      const isac::CutWindow::RowCol rc = w.row_col_of(c.cut);
      eq(e.name, "row_col_of.row", rc.row, c.row); eq(e.name, "row_col_of.col", rc.col, c.col);
      eq(e.name, "cut_of", w.cut_of(c.row - e.cf.row0, c.col - e.cf.col0), c.cut);
    }
    // round trip over the whole zone, in the order cfar2D.m:23-24 lists the CUTs: columns slowest, rows fastest, ordinals 0, 1, 2, ...
    int next = 0;
    for (int col = e.cf.col0; col <= e.cf.col1; ++col)
      for (int row = e.cf.row0; row <= e.cf.row1; ++row, ++next) {
        const int cut = w.cut_of(row - e.cf.row0, col - e.cf.col0);
        const isac::CutWindow::RowCol rc = w.row_col_of(cut);
        if (cut != next || rc.row != row || rc.col != col) {
          std::fprintf(stderr, "%s: (row %d, col %d) -> CUT %d (expected %d) -> (row %d, col %d)\n", e.name, row, col, cut, next, rc.row, rc.col);
          ++failures;
        }
      }
    eq(e.name, "CUTs visited", next, e.n_cut);
  }
  // fft2D.m:77-82 with rRes = 1.25 m, vRes = 4.5 m/s, nFFT = 256 (every product exact in binary floating point)
  isac_est_params ep{};
  ep.n_ifft = 4096; ep.n_fft = 256; ep.r_res = 1.25; ep.v_res = 4.5;
  eqd("estimates", "range_of(1)", isac::CutWindow::range_of(1, ep), 0.0);
  eqd("estimates", "range_of(42)", isac::CutWindow::range_of(42, ep), 51.25);
  eqd("estimates", "range_of(411)", isac::CutWindow::range_of(411, ep), 512.5);
  eqd("estimates", "velocity_of(129)", isac::CutWindow::velocity_of(129, ep), 0.0);
  eqd("estimates", "velocity_of(118)", isac::CutWindow::velocity_of(118, ep), -49.5);
  eqd("estimates", "velocity_of(140)", isac::CutWindow::velocity_of(140, ep), 49.5);
  ep.n_fft = 16; ep.v_res = 0.5;
  eqd("estimates", "velocity_of(1), nFFT 16", isac::CutWindow::velocity_of(1, ep), -4.0);
  eqd("estimates", "velocity_of(16), nFFT 16", isac::CutWindow::velocity_of(16, ep), 3.5);
  if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  std::printf("cut_window: %d configurations OK\n", (int)(sizeof(kCases) / sizeof(kCases[0])));
  return 0;
}
