// The MEX gateway's 'fft2DTargets' command (mex/matlab/+sensing/+estimation/targetList.m), linked against the in-process mx runtime of tests/mex_runtime/ (with its
// struct-array extension mx_struct_array.cpp) and libisac_hip.so and CALLED through mexFunction the way the shim calls it (tests/test_gpu_target_list.py reads the result).
//   mex_targets_host <in.bin> <out.bin>
// in:  int32 K, L, A, nIFFT, nFFT, guard[2], train[2], row0, row1, col0, col1, pad;  double rRes, vRes, Pfa, azimuthScanScale, azimuthScanGranularity;
//      rxGrid, txGrid [K x L x A] (interleaved complex, column-major)
// out: int32 n, then n doubles each of rng, vel, azi, power, hits, row, col;  stdout: the error identifier of a call before any fft2D
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "isac.h"
#include "mex_runtime/mx_runtime.hpp"

namespace {
struct hdr_t { int32_t K, L, A, n_ifft, n_fft, guard[2], train[2], row0, row1, col0, col1, pad; double r_res, v_res, pfa, az_scale, az_gran; };
void rd(void* p, size_t n, FILE* f) { if (std::fread(p, 1, n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(3); } }
mxArray* scalar(double v) { return mxCreateDoubleScalar(v); }
mxArray* row2(double a, double b) { mxArray* m = mxCreateDoubleMatrix(1, 2, mxREAL); mxGetDoubles(m)[0] = a; mxGetDoubles(m)[1] = b; return m; }
mxArray* cplx_array(const std::vector<isac_c64>& v, mwSize d0, mwSize d1, mwSize d2) {
  const mwSize dims[3] = {d0, d1, d2};
  mxArray* a = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxCOMPLEX);
  std::memcpy(mxGetComplexDoubles(a), v.data(), sizeof(isac_c64) * d0 * d1 * d2);
  return a;
}
mxArray* make_struct(std::vector<std::pair<const char*, mxArray*>> f) {
  std::vector<const char*> names;
  for (auto& kv : f) names.push_back(kv.first);
  mxArray* s = mxCreateStructMatrix(1, 1, (int)names.size(), names.data());
  for (auto& kv : f) mxSetField(s, 0, kv.first, kv.second);
  return s;
}
mxArray* call(const char* name, std::vector<const mxArray*> args) {
  mxArray* nm = mxr_string(name);
  std::vector<const mxArray*> prhs{nm};
  prhs.insert(prhs.end(), args.begin(), args.end());
  mxArray* plhs[2] = {nullptr, nullptr};
  try { mexFunction(1, plhs, (int)prhs.size(), prhs.data()); } catch (...) { mxr_destroy(nm); throw; }
  mxr_destroy(nm);
  return plhs[0];
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: mex_targets_host <in.bin> <out.bin>\n"); return 1; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 1; }
  hdr_t h;
  rd(&h, sizeof(h), f);
  const size_t ng = (size_t)h.K * h.L * h.A;
  std::vector<isac_c64> rx(ng), tx(ng);
  rd(rx.data(), sizeof(isac_c64) * ng, f); rd(tx.data(), sizeof(isac_c64) * ng, f);
  std::fclose(f);
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) { std::perror(argv[2]); return 1; }
  try {
    std::string before;
    try { call("fft2DTargets", {}); } catch (const MexError& e) { before = e.id; }               // no completed fft2D yet
    std::printf("%s\n", before.c_str());
    // radarEstParams (radarParams.m:69-78,140-144) and cfar2D's output (cfar2D.m:23-37), as MATLAB hands them over
    mxArray* rp = make_struct({{"nIFFT", scalar(h.n_ifft)}, {"nFFT", scalar(h.n_fft)}, {"rRes", scalar(h.r_res)}, {"vRes", scalar(h.v_res)},
                               {"azimuthScanScale", scalar(h.az_scale)}, {"azimuthScanGranularity", scalar(h.az_gran)}, {"elevationScanScale", scalar(180)},
                               {"elevationScanGranularity", scalar(1)}, {"antennaType", mxr_object("parameters.baseStation.antenna.ula")}});
    const int n_rows = h.row1 - h.row0 + 1, n_cols = h.col1 - h.col0 + 1;
    mxArray* cut = mxCreateDoubleMatrix(2, (mwSize)n_rows * n_cols, mxREAL);                     // rows fastest (cfar2D.m:23-24)
    for (int c = 0, i = 0; c < n_cols; ++c)
      for (int r = 0; r < n_rows; ++r, ++i) { mxGetDoubles(cut)[2 * i] = h.row0 + r; mxGetDoubles(cut)[2 * i + 1] = h.col0 + c; }
    mxArray* det = mxr_object("phased.CFARDetector2D");
    mxr_set_property(det, "ProbabilityFalseAlarm", scalar(h.pfa));
    mxr_set_property(det, "GuardBandSize", row2(h.guard[0], h.guard[1]));
    mxr_set_property(det, "TrainingBandSize", row2(h.train[0], h.train[1]));
    mxArray* cfar = make_struct({{"CUTIdx", cut}, {"cfarDetector2D", det}});
    call("fft2D", {rp, cfar, cplx_array(rx, h.K, h.L, h.A), cplx_array(tx, h.K, h.L, h.A)});     // fft2D.m:1 with MATLAB arrays
    mxArray* t = call("fft2DTargets", {});                                                        // targetList.m
    if (!mxIsStruct(t) || (mxGetNumberOfElements(t) && mxGetN(t) != 1)) { std::fprintf(stderr, "fft2DTargets: not an [n x 1] struct array\n"); return 4; }
    const int32_t n = (int32_t)mxGetNumberOfElements(t);
    std::fwrite(&n, sizeof(n), 1, o);
    for (const char* name : {"rng", "vel", "azi", "power", "hits", "row", "col"})
      for (int32_t i = 0; i < n; ++i) {
        const mxArray* v = mxGetField(t, (mwIndex)i, name);
        if (!v || mxGetNumberOfElements(v) != 1) { std::fprintf(stderr, "fft2DTargets: element %d has no scalar field %s\n", (int)i, name); return 4; }
        const double d = mxGetScalar(v);
        std::fwrite(&d, sizeof(d), 1, o);
      }
  } catch (const MexError& e) {
    std::fprintf(stderr, "%s: %s\n", e.id.c_str(), e.msg.c_str());
    return 2;
  }
  std::fclose(o);
  mxr_run_at_exit();
  return 0;
}
