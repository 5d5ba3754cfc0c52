// The rest of applyChannelModel (uePhy.m:724-755 downlink, gNBPhy.m:833-864 uplink) behind the channel object:
//   rxWaveform = db2mag(-pathLoss) * rxWaveform;                                uePhy.m:742-748   gNBPhy.m:851-857
//   rxWaveform = rxWaveform .* 10.^(RxGain/20);                                 uePhy.m:935-940   gNBPhy.m:1064-1069
//   rxWaveform = rxWaveform + sqrt(Nt/2)*complex(randn, randn)                  uePhy.m:942-950   gNBPhy.m:1071-1080
// Host side: the scalars those lines take (TR 38.901 7.4.1 path loss = nrPathLoss as config5GNRModels.m calls it, fspl, the thermal-noise power, the DFT matrix of a link
// without a CDL object) -- plain C, no context.  Device side: ONE streaming kernel over a batch of received waveforms, in place.
#include "isac_internal.hpp"
#include "echo_dev.hpp"

using namespace isac;

// ---------------------------------------------------------------- host scalars
namespace {

constexpr double kLightSpeed = 299792458.0;        // physconst('LightSpeed')
constexpr double kBoltzmann = 1.380649e-23;        // physconst('Boltzmann')
constexpr double kPi = 3.14159265358979323846;

// TR 38.901 V16 Table 7.4.1-1, mean path loss.  d: d3D [m], d2: d2D [m], f: fc [GHz], hb / hu: h_BS / h_UT [m] (third coordinate of the first / second position).
// Evaluated for any distance: the table's ranges of validity are not enforced (nrPathLoss does not either).
double pl_uma_umi_los(bool uma, double d, double d2, double f, double fc_hz, double hb, double hu, double he) {
  const double dbp = 4.0 * (hb - he) * (hu - he) * fc_hz / kLightSpeed;          // d'BP
  const double a = uma ? 28.0 : 32.4, n1 = uma ? 22.0 : 21.0, c2 = uma ? 9.0 : 9.5;
  if (d2 <= dbp) return a + n1 * std::log10(d) + 20.0 * std::log10(f);
  return a + 40.0 * std::log10(d) + 20.0 * std::log10(f) - c2 * std::log10(dbp * dbp + (hb - hu) * (hb - hu));
}
double pl_rma_pl1(double d, double f, double h) {
  return 20.0 * std::log10(40.0 * kPi * d * f / 3.0) + std::fmin(0.03 * std::pow(h, 1.72), 10.0) * std::log10(d) - std::fmin(0.044 * std::pow(h, 1.72), 14.77) +
         0.002 * std::log10(h) * d;
}
double pl_rma_los(double d, double d2, double f, double fc_hz, double hb, double hu, double h) {
  const double dbp = 2.0 * kPi * hb * hu * fc_hz / kLightSpeed;                  // dBP
  if (d2 <= dbp) return pl_rma_pl1(d, f, h);
  return pl_rma_pl1(dbp, f, h) + 40.0 * std::log10(d / dbp);
}

}  // namespace

extern "C" int isac_path_loss_38901(int32_t scenario, double fc_hz, int32_t los, const double* bs_pos, const double* ue_pos, const isac_path_loss_config* cfg,
                                    double* pl_db) {
  if (!bs_pos || !ue_pos || !pl_db || !(fc_hz > 0.0) || scenario < ISAC_PL_UMA || scenario > ISAC_PL_INF_HH) return ISAC_ERR_INVALID_ARG;
  if (bs_pos[0] == ue_pos[0] && bs_pos[1] == ue_pos[1] && bs_pos[2] == ue_pos[2]) { *pl_db = 0.0; return ISAC_OK; }   // config5GNRModels.m:32-33: not -Inf
  const double h = cfg ? cfg->building_height : 5.0, W = cfg ? cfg->street_width : 20.0, he = cfg ? cfg->environment_height : 1.0;
  const bool opt = cfg && cfg->optional_model != 0;
  const double dx = ue_pos[0] - bs_pos[0], dy = ue_pos[1] - bs_pos[1], hb = bs_pos[2], hu = ue_pos[2];
  const double d2 = std::sqrt(dx * dx + dy * dy), d = std::sqrt(d2 * d2 + (hb - hu) * (hb - hu)), f = fc_hz / 1e9;
  const double lf = std::log10(f), ld = std::log10(d);
  double pl_los = 0.0, pl_n = 0.0;               // LoS formula; NLoS PL' (the result is max(LoS, PL') unless noted)
  bool n_is_final = false;                       // optional models: taken as they stand
  switch (scenario) {
    case ISAC_PL_UMA:
      pl_los = pl_uma_umi_los(true, d, d2, f, fc_hz, hb, hu, he);
      if (opt) { pl_n = 32.4 + 20.0 * lf + 30.0 * ld; n_is_final = true; }
      else pl_n = 13.54 + 39.08 * ld + 20.0 * lf - 0.6 * (hu - 1.5);
      break;
    case ISAC_PL_UMI:
      pl_los = pl_uma_umi_los(false, d, d2, f, fc_hz, hb, hu, he);
      if (opt) { pl_n = 32.4 + 20.0 * lf + 31.9 * ld; n_is_final = true; }
      else pl_n = 35.3 * ld + 22.4 + 21.3 * lf - 0.3 * (hu - 1.5);
      break;
    case ISAC_PL_RMA: {
      pl_los = pl_rma_los(d, d2, f, fc_hz, hb, hu, h);
      const double lhb = std::log10(hb), l11 = std::log10(11.75 * hu);
      pl_n = 161.04 - 7.1 * std::log10(W) + 7.5 * std::log10(h) - (24.37 - 3.7 * (h / hb) * (h / hb)) * lhb + (43.42 - 3.1 * lhb) * (ld - 3.0) + 20.0 * lf -
             (3.2 * l11 * l11 - 4.97);
      break;
    }
    case ISAC_PL_INH:
      pl_los = 32.4 + 17.3 * ld + 20.0 * lf;
      if (opt) { pl_n = 32.4 + 20.0 * lf + 31.9 * ld; n_is_final = true; }
      else pl_n = 38.3 * ld + 17.30 + 24.9 * lf;
      break;
    default: {                                   // InF-*
      pl_los = 31.84 + 21.50 * ld + 19.00 * lf;
      const double sl = 33.0 + 25.5 * ld + 20.0 * lf;
      if (scenario == ISAC_PL_INF_SL) pl_n = sl;
      else if (scenario == ISAC_PL_INF_DL) pl_n = std::fmax(18.6 + 35.7 * ld + 20.0 * lf, sl);
      else if (scenario == ISAC_PL_INF_SH) pl_n = 32.4 + 23.0 * ld + 20.0 * lf;
      else if (scenario == ISAC_PL_INF_DH) pl_n = 33.63 + 21.9 * ld + 20.0 * lf;
      else pl_n = pl_los;                        // InF-HH: the LoS formula whatever `los` says
      break;
    }
  }
  *pl_db = los ? pl_los : (n_is_final ? pl_n : std::fmax(pl_los, pl_n));
  return ISAC_OK;
}

extern "C" int isac_path_loss_fspl(double fc_hz, const double* bs_pos, const double* ue_pos, double* pl_db) {
  if (!bs_pos || !ue_pos || !pl_db || !(fc_hz > 0.0)) return ISAC_ERR_INVALID_ARG;
  const double dx = ue_pos[0] - bs_pos[0], dy = ue_pos[1] - bs_pos[1], dz = ue_pos[2] - bs_pos[2];
  const double R = std::sqrt(dx * dx + dy * dy + dz * dz), lambda = kLightSpeed / fc_hz;
  const double L = 20.0 * std::log10(4.0 * kPi * R / lambda);                    // R = 0: -Inf
  *pl_db = L < 0.0 ? 0.0 : L;                                                    // fspl: "L(L < 0) = 0"
  return ISAC_OK;
}

extern "C" int isac_thermal_noise_power(double temperature_k, double noise_figure_db, double sample_rate_hz, double* nt_w) {
  if (!nt_w) return ISAC_ERR_INVALID_ARG;
  const double nf = std::pow(10.0, noise_figure_db / 10.0);                      // uePhy.m:945
  *nt_w = kBoltzmann * (temperature_k + 290.0 * (nf - 1.0)) * sample_rate_hz;    // uePhy.m:947
  return ISAC_OK;
}

extern "C" int isac_dft_channel_matrix(int32_t Nt, int32_t Nr, isac_c64* H) {
  if (!H || Nt <= 0 || Nr <= 0) return ISAC_ERR_INVALID_ARG;
  // norm(H) is the spectral norm.  The slice keeps whole rows (Nt <= Nr = n) or whole columns (Nr <= Nt = n) of the n-point DFT matrix: they are orthogonal and of
  // length sqrt(n), so H H' (or H' H) = n I and every singular value is sqrt(n) exactly -- no SVD needed.
  const long long n = Nt > Nr ? Nt : Nr;
  const double inv = 1.0 / std::sqrt((double)n);
  for (long long r = 0; r < Nr; ++r)
    for (long long t = 0; t < Nt; ++t) {
      const double ang = 2.0 * kPi * (double)((t * r) % n) / (double)n;
      H[t + (long long)Nt * r] = isac_c64{std::cos(ang) * inv, -std::sin(ang) * inv};
    }
  return ISAC_OK;
}

// ---------------------------------------------------------------- the device kernel
// Memory-bound streaming over n_jobs x T x Nr elements of 16 B, in place: one 128-bit load and one 128-bit store per element (two loads in the injected mode), no LDS,
// no scratch.  A flat grid over (job, block of kRxfeBlock elements): the batch is one index space, so 40 downlink jobs of [61 909 x 2] fill the device as well as 10 uplink
// jobs of [61 909 x 64] do.  Each thread keeps kRxfeU elements in flight (all loads issued before the first use); the flat launch with few elements per thread is the
// shape that copies fastest on this part (profiles/r05_cbench_copy_rate.txt: 6.2 TB/s against 5.0-5.9 for persistent grids).  No alignment assumption beyond the 16 B of an
// element: the index is the element's own, odd T and Nr = 1 need nothing special.
// Per element, in the reference's order: y = fma(sig, w, (y * path_scale) * gain_scale), sig = sqrt(Nt / 2) formed once on the host.
namespace {

struct RxfeJob {                 // device image of isac_rx_frontend_job
  c64* y;
  const c64* w;
  double s1, s2, sig;
  unsigned long long seed;
};
constexpr int kRxfeU = 2, kRxfeBlock = 256 * kRxfeU;

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) f64x2 gc64;           // the table's pointers are global memory: global_load / global_store_dwordx4, not the flat forms

template <int MODE>              // isac_noise_mode: 0 none, 1 injected, 2 Philox
__global__ __launch_bounds__(256) void rxfe_kernel(const RxfeJob* __restrict__ jobs, long long n, unsigned blocks_per_job) {
  const unsigned job = blockIdx.x / blocks_per_job, blk = blockIdx.x - job * blocks_per_job;
  const RxfeJob jb = jobs[job];                                  // workgroup-uniform: scalar loads
  gc64* y = (gc64*)jb.y;
  const gc64* wn = (const gc64*)jb.w;
  const long long e0 = (long long)blk * kRxfeBlock + threadIdx.x;
  c64 v[kRxfeU], w[kRxfeU];
#pragma unroll
  for (int u = 0; u < kRxfeU; ++u) {                             // every load is issued before the first use; past the end a lane re-reads the last element (no branch
    const long long e = e0 + 256 * u, ec = e < n ? e : n - 1;    // around a load) and stores nothing
    const f64x2 a = y[ec];
    v[u] = c64{a.x, a.y};
    if (MODE == ISAC_NOISE_INJECTED) { const f64x2 b = wn[ec]; w[u] = c64{b.x, b.y}; }
  }
#pragma unroll
  for (int u = 0; u < kRxfeU; ++u) {
    const long long e = e0 + 256 * u;
    if (MODE == ISAC_NOISE_PHILOX) w[u] = philox_normal_pair((uint64_t)e, jb.seed, kRxFrontEndStream);
    c64 r = (v[u] * jb.s1) * jb.s2;
    if (MODE != ISAC_NOISE_NONE) r = c64{::fma(jb.sig, w[u].re, r.re), ::fma(jb.sig, w[u].im, r.im)};
    if (e < n) y[e] = f64x2{r.re, r.im};
  }
}

}  // namespace

int isac_rx_frontend_jobs(isac_ctx* ctx, const isac_rx_frontend_job* jobs, int n_jobs, long long T, int Nr, int noise_mode) {
  if (!jobs) return fail(ctx, ISAC_ERR_INVALID_ARG, "rx front end: NULL job table");
  if (n_jobs <= 0 || T <= 0 || Nr <= 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "rx front end: bad dimensions (n_jobs, T, Nr must be positive)");
  if (noise_mode != ISAC_NOISE_NONE && noise_mode != ISAC_NOISE_INJECTED && noise_mode != ISAC_NOISE_PHILOX)
    return fail(ctx, ISAC_ERR_INVALID_ARG, "rx front end: noise_mode must be ISAC_NOISE_NONE, _INJECTED or _PHILOX (the spectral modes belong to monoStaticSensing)");
  const long long n = T * (long long)Nr;
  const long long bpj = (n + kRxfeBlock - 1) / kRxfeBlock;
  if (bpj * n_jobs >= (1ll << 31)) return fail(ctx, ISAC_ERR_CAPACITY, "rx front end: more than 2^31 element blocks in one batch");
  for (int j = 0; j < n_jobs; ++j) {
    if (!jobs[j].d_y) return fail(ctx, ISAC_ERR_INVALID_ARG, "rx front end: job without an array");
    if (noise_mode == ISAC_NOISE_INJECTED && !jobs[j].d_noise_unit) return fail(ctx, ISAC_ERR_INVALID_ARG, "rx front end: ISAC_NOISE_INJECTED without a noise buffer");
    if (!(jobs[j].noise_power >= 0.0)) return fail(ctx, ISAC_ERR_INVALID_ARG, "rx front end: negative (or NaN) noise power");
  }
  const size_t bytes = sizeof(RxfeJob) * (size_t)n_jobs;
  ISAC_TRY(ensure(ctx, ctx->rxfe_tab, bytes));
  void* h = nullptr;
  ISAC_TRY(stage_acquire(ctx, bytes, &h));
  RxfeJob* tab = (RxfeJob*)h;
  for (int j = 0; j < n_jobs; ++j) {
    tab[j] = RxfeJob{(c64*)jobs[j].d_y, (const c64*)jobs[j].d_noise_unit, jobs[j].path_scale, jobs[j].gain_scale, std::sqrt(jobs[j].noise_power / 2.0), jobs[j].seed};
    ctx->range_cache.touch(jobs[j].d_y, sizeof(c64) * (size_t)n);        // an array that overlaps a cached grid drops the cached range rows
  }
  ISAC_TRY(stage_commit(ctx, ctx->rxfe_tab.p, bytes));
  const dim3 grid((unsigned)(bpj * n_jobs)), block(256);
  const RxfeJob* d_tab = (const RxfeJob*)ctx->rxfe_tab.p;
  switch (noise_mode) {
    case ISAC_NOISE_NONE: hipLaunchKernelGGL(rxfe_kernel<ISAC_NOISE_NONE>, grid, block, 0, ctx->stream, d_tab, n, (unsigned)bpj); break;
    case ISAC_NOISE_INJECTED: hipLaunchKernelGGL(rxfe_kernel<ISAC_NOISE_INJECTED>, grid, block, 0, ctx->stream, d_tab, n, (unsigned)bpj); break;
    default: hipLaunchKernelGGL(rxfe_kernel<ISAC_NOISE_PHILOX>, grid, block, 0, ctx->stream, d_tab, n, (unsigned)bpj); break;
  }
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}

extern "C" int isac_rx_frontend_batch_dev(isac_ctx* ctx, const isac_rx_frontend_job* jobs, int32_t n_jobs, int64_t T, int32_t Nr, int32_t noise_mode) {
  ISAC_ENTER(ctx);
  return isac_rx_frontend_jobs(ctx, jobs, n_jobs, T, Nr, noise_mode);
}

extern "C" int isac_rx_frontend_dev(isac_ctx* ctx, isac_c64* d_y, int64_t T, int32_t Nr, double path_scale, double gain_scale, double noise_power, int32_t noise_mode,
                                    const isac_c64* d_noise_unit, uint64_t seed) {
  ISAC_ENTER(ctx);
  const isac_rx_frontend_job job{d_y, d_noise_unit, path_scale, gain_scale, noise_power, seed};
  return isac_rx_frontend_jobs(ctx, &job, 1, T, Nr, noise_mode);
}
