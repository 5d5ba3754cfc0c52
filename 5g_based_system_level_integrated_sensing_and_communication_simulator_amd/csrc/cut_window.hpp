// The CUT window of one fft2D call: the rectangle of cells under test that cfar2D.m:17-24 builds, widened by guard + training cells on every side -- the part of the
// range-Doppler map the CFAR stage reads (ctx->pwin [nr x nc x A]).  Host-side, plain C++ (include/isac.h and nothing else: a host compiler builds and tests it).
// Every unit takes the window's numbers from here; the structs the kernels take by value (CfarGeom, TailGeom, WinGeom) are filled from it.
#pragma once
#include "../../include/isac.h"

namespace isac {
struct CutWindow {
  int row0, col0;               // first CUT row / column of the map, 1-based
  int gr, gc, hr, hc;           // guard / guard + training half sizes
  int n_cut_rows, n_cut_cols;
  int nr, nc;                   // window dims: the CUT zone + hr (hc) cells on both sides
  int first_row, first_col;     // map row / column of window element (0, 0), 1-based
  static CutWindow of(const isac_cfar_config& cf) {
    CutWindow w{};
    w.row0 = cf.row0; w.col0 = cf.col0; w.gr = cf.guard[0]; w.gc = cf.guard[1];
    w.hr = cf.guard[0] + cf.train[0]; w.hc = cf.guard[1] + cf.train[1];
    w.n_cut_rows = cf.row1 - cf.row0 + 1; w.n_cut_cols = cf.col1 - cf.col0 + 1;
    w.nr = w.n_cut_rows + 2 * w.hr; w.nc = w.n_cut_cols + 2 * w.hc; w.first_row = cf.row0 - w.hr; w.first_col = cf.col0 - w.hc;
    return w;
  }
  template <class Geom> void fill(Geom& g) const { g.nr = nr; g.nc = nc; g.hr = hr; g.hc = hc; g.gr = gr; g.gc = gc; g.n_cut_rows = n_cut_rows; g.n_cut_cols = n_cut_cols; }   // a kernel's by-value geometry
  long long n_cut() const { return (long long)n_cut_rows * n_cut_cols; }
  // CUT ordinal: rows fastest (cfar2D.m:23-24, the order phased.CFARDetector2D reports); cr, cc 0-based inside the zone; RowCol: of the map, 1-based
  int cut_of(int cr, int cc) const { return cr + n_cut_rows * cc; }
  struct RowCol { int row, col; };
  RowCol row_col_of(int cut) const { return RowCol{row0 + cut % n_cut_rows, col0 + cut / n_cut_rows}; }
  static double range_of(int row, const isac_est_params& ep) { return (double)(row - 1) * ep.r_res; }                          // of a 1-based map row: fft2D.m:77,:81
  static double velocity_of(int col, const isac_est_params& ep) { return ((double)col - ep.n_fft / 2.0 - 1.0) * ep.v_res; }    // of a 1-based map column: fft2D.m:78,:82
};
}  // namespace isac
