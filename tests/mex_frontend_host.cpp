// The MEX gateway's commands for the tail of applyChannelModel ('pathLoss', 'thermalNoisePower', 'rxFrontEnd', 'size'), linked against the in-process mx runtime of
// tests/mex_runtime/ and libisac_hip.so and CALLED the way the shims under mex/matlab/+communication/ call them (tests/test_gpu_rx_frontend.py reads the results).
//   mex_frontend_host <in.bin> <out.bin>
// in:  int64 T, Nr;  double pathLoss_dB, rxGain_dB, temperature, noiseFigure_dB, sampleRate, fc, bs[3], ue[3];  y [T x Nr], w [T x Nr] (interleaved complex, column-major)
// out: 19 doubles (9 scenarios x LoS, NLoS; fspl), Nt, then three [T x Nr] arrays: MATLAB array + injected noise, device handle in place + injected noise, noiseless
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "isac.h"
#include "mex_runtime/mx_runtime.hpp"

namespace {
void rd(void* p, size_t n, FILE* f) { if (std::fread(p, 1, n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(3); } }
mxArray* row3(const double* v) { mxArray* a = mxCreateDoubleMatrix(1, 3, mxREAL); std::memcpy(mxGetDoubles(a), v, 3 * sizeof(double)); return a; }
mxArray* cplx_mat(const std::vector<isac_c64>& v, mwSize m, mwSize n) {
  mxArray* a = mxCreateDoubleMatrix(m, n, mxCOMPLEX);
  std::memcpy(mxGetComplexDoubles(a), v.data(), sizeof(isac_c64) * m * n);
  return a;
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
std::string error_id(const char* name, std::vector<const mxArray*> args) {
  try { call(name, args); } catch (const MexError& e) { return e.id; }
  return "";
}
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { std::fprintf(stderr, "usage: mex_frontend_host <in.bin> <out.bin>\n"); return 1; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 1; }
  int64_t dims[2];
  double p[12];
  rd(dims, sizeof(dims), f); rd(p, sizeof(p), f);
  const mwSize T = (mwSize)dims[0], Nr = (mwSize)dims[1];
  std::vector<isac_c64> y(T * Nr), w(T * Nr);
  rd(y.data(), sizeof(isac_c64) * y.size(), f); rd(w.data(), sizeof(isac_c64) * w.size(), f);
  std::fclose(f);
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) { std::perror(argv[2]); return 1; }
  try {
    mxArray *bs = row3(p + 6), *ue = row3(p + 9), *fc = mxCreateDoubleScalar(p[5]);
    static const char* names[] = {"UMa", "UMi", "RMa", "InH", "InF-SL", "InF-DL", "InF-SH", "InF-DH", "InF-HH"};
    for (const char* s : names)
      for (double los : {1.0, 0.0}) {                                  // config5GNRModels.m's shim: (char, fc, los, bs, ue)
        const double v = mxGetScalar(call("pathLoss", {mxr_string(s), fc, mxCreateDoubleScalar(los), bs, ue}));
        std::fwrite(&v, sizeof(v), 1, o);
      }
    double v = mxGetScalar(call("pathLoss", {mxr_string("fspl"), fc, mxr_empty(), bs, ue}));      // configFreeSpaceModel.m's shim
    std::fwrite(&v, sizeof(v), 1, o);
    mxArray* nt = call("thermalNoisePower", {mxCreateDoubleScalar(p[2]), mxCreateDoubleScalar(p[3]), mxCreateDoubleScalar(p[4])});
    v = mxGetScalar(nt);
    std::fwrite(&v, sizeof(v), 1, o);
    mxArray *pl = mxCreateDoubleScalar(p[0]), *g = mxCreateDoubleScalar(p[1]), *ym = cplx_mat(y, T, Nr), *wm = cplx_mat(w, T, Nr);
    // applyRxFrontEnd.m with a MATLAB array: array in, array out, MATLAB's randn as injected noise
    mxArray* r1 = call("rxFrontEnd", {ym, pl, g, nt, wm});
    if (mxGetM(r1) != T || mxGetN(r1) != Nr) { std::fprintf(stderr, "rxFrontEnd: wrong output size\n"); return 4; }
    std::fwrite(mxGetComplexDoubles(r1), sizeof(isac_c64), T * Nr, o);
    // ... with a device handle: in place, the same handle comes back
    mxArray* h = call("toDevice", {ym});
    mxArray* sz = call("size", {h});
    if (mxGetNumberOfElements(sz) != 2 || mxGetDoubles(sz)[0] != (double)T || mxGetDoubles(sz)[1] != (double)Nr) { std::fprintf(stderr, "size: wrong dims\n"); return 4; }
    mxArray* h2 = call("rxFrontEnd", {h, pl, g, nt, wm});
    if (*mxGetUint64s(h2) != *mxGetUint64s(h)) { std::fprintf(stderr, "rxFrontEnd: a handle must come back as itself\n"); return 4; }
    mxArray* r2 = call("gather", {h2});
    std::fwrite(mxGetComplexDoubles(r2), sizeof(isac_c64), T * Nr, o);
    call("free", {h});
    // noiseless
    mxArray* r3 = call("rxFrontEnd", {ym, pl, g, nt});
    std::fwrite(mxGetComplexDoubles(r3), sizeof(isac_c64), T * Nr, o);
    // error identifiers
    std::printf("%s %s\n", error_id("pathLoss", {mxr_string("UMx"), fc, mxCreateDoubleScalar(1.0), bs, ue}).c_str(),
                error_id("rxFrontEnd", {ym, pl, g, nt, cplx_mat(w, T - 1, Nr)}).c_str());
  } catch (const MexError& e) {
    std::fprintf(stderr, "%s: %s\n", e.id.c_str(), e.msg.c_str());
    return 2;
  }
  std::fclose(o);
  mxr_run_at_exit();
  return 0;
}
