// Target tracking across CPIs (gfx950 only): isac_track_state_bytes, isac_track_reset_dev, isac_track_step_dev, isac_track_get_dev (include/isac_track.h has the
// definition; project-defined).
//   track_step_kernel   one scan of every bank: predict, the groups' greedy association with the sequential scalar EKF updates, bookkeeping, births
// One workgroup per bank, 256 threads (four wave64), thread t owns slot t: the slot's x [4] and P [16] are loaded once, stay in the thread's registers for the whole scan and
// are stored once.  A group's measurements (at most 256 records of 72 bytes, 18 KB) are staged in LDS; a thread whose track is live and has no measurement of the group yet
// walks them and keeps its BEST pair (smallest d^2 within the gate, the lower measurement on a tie).  A greedy round is a block-wide argmin over the threads' bests on the key
// (d^2, slot): shuffles inside a wave, then the four waves' values through LDS, read by every thread (all take the same branch).  The winner applies the update for real,
// claims the measurement and leaves the group.  CACHED BESTS: the d^2 ROW OF A TRACK IS RECOMPUTED, NOT KEPT -- only a thread whose cached best was the claimed measurement
// walks the group again (over the measurements still free); everybody else's best is still its best, because the d^2 of other tracks do not change when one track is
// updated, and a recomputed d^2 is the same bits as the first one (the same code on the same registers).  A kept row would be T x 256 doubles per bank: 512 KB, more than
// the LDS, and a round trip through global memory per round.  The cost is the serial rounds: at most min(tracks, measurements) of them per group, each one argmin (two
// barriers) plus the losers' walks.
// Births need the bank-wide order of the unassigned fixes: every group appends its own (a ballot prefix sum) to an LDS list of at most 256 -- later ones cannot find a slot
// whatever the table holds -- and after the bookkeeping the r-th free slot takes the r-th entry.  No atomics, nothing shared between banks, a strict total order in every
// round: the same bits on every run.  All stores are plain vector stores.
#include <cmath>
#include <vector>

#include "isac_internal.hpp"
#include "cpi_post.hpp"
#include "../../include/isac_track.h"

namespace isac {

constexpr int kTrkBlock = 256;
constexpr double kTrkRadToDeg = 57.29577951308232087679815481410517;

struct TrkNode { double x, y, z; };
struct TrkLink { int tx, rx; };
struct TrkMeas { double z[4]; double var[4]; int kind, link; };           // var = sigma^2
static_assert(sizeof(TrkMeas) == 72, "a group of 256 is staged as 18 KB");
struct TrkGroup { int first, end; };                                      // measurements first .. end - 1, indices into the M given
struct TrkPar { double dt, q, gate2, v02, height; int confirm_hits, tent_misses, max_misses, T; };   // q = sigma_acc^2, v02 = init_v0^2

// The state block, carved in this order (every array 16-byte aligned): the table of include/isac_track.h, then the banks' id counters.
struct TrkState { int *status, *id, *age, *hits, *misses, *dof; double *x, *P, *nis; int* next_id; size_t bytes; };
static TrkState trk_state(void* base, int B, int T) {
  Carver cv;
  const size_t n = (size_t)B * T;
  char* p = (char*)base;
  TrkState s;
  s.status = (int*)(p + cv.take(sizeof(int) * n)); s.id = (int*)(p + cv.take(sizeof(int) * n)); s.age = (int*)(p + cv.take(sizeof(int) * n));
  s.hits = (int*)(p + cv.take(sizeof(int) * n)); s.misses = (int*)(p + cv.take(sizeof(int) * n)); s.dof = (int*)(p + cv.take(sizeof(int) * n));
  s.x = (double*)(p + cv.take(sizeof(double) * 4 * n)); s.P = (double*)(p + cv.take(sizeof(double) * 16 * n)); s.nis = (double*)(p + cv.take(sizeof(double) * n));
  s.next_id = (int*)(p + cv.take(sizeof(int) * (size_t)B));
  s.bytes = (cv.total + 255) & ~(size_t)255;
  return s;
}

struct Trk { double x[4]; double P[16]; };

// One scalar component (include/isac_track.h, step 3): returns nu^2 / s.
__device__ __forceinline__ double trk_component(Trk& t, const double (&H)[4], double nu, double var) {
  double PH[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double a = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) a += t.P[4 * i + j] * H[j];
    PH[i] = a;
  }
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) s += H[i] * PH[i];
  s += var;
  double K[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { K[i] = PH[i] / s; t.x[i] += K[i] * nu; }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) t.P[4 * i + j] -= K[i] * PH[j];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = i + 1; j < 4; ++j) { const double m = 0.5 * (t.P[4 * i + j] + t.P[4 * j + i]); t.P[4 * i + j] = m; t.P[4 * j + i] = m; }
  return nu * nu / s;
}

// g = (u_tx + u_rx)_xy and the range sum at the track's position
__device__ __forceinline__ void trk_geom(const Trk& t, const TrkNode& pt, const TrkNode& pr, double height, double& gx, double& gy, double& rsum) {
  const double ax = t.x[0] - pt.x, ay = t.x[1] - pt.y, az = height - pt.z, bx = t.x[0] - pr.x, by = t.x[1] - pr.y, bz = height - pr.z;
  const double da = sqrt(ax * ax + ay * ay + az * az), db = sqrt(bx * bx + by * by + bz * bz);
  gx = 0.0; gy = 0.0;
  if (da != 0.0) { gx += ax / da; gy += ay / da; }
  if (db != 0.0) { gx += bx / db; gy += by / db; }
  rsum = da + db;
}

// The measurement applied to t (a copy: the virtual update; the slot itself: the real one): d^2, and the number of components applied into *n_comp.
__device__ __forceinline__ double trk_apply(Trk& t, const TrkMeas& m, const TrkNode* __restrict__ nodes, const TrkLink* __restrict__ links, double height, int* n_comp) {
  double d2 = 0.0;
  int n = 0;
  if (m.kind == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (m.z[c] == m.z[c]) {                                              // not NaN (x and y never are)
        double H[4] = {0.0, 0.0, 0.0, 0.0};
        H[c] = 1.0;
        d2 += trk_component(t, H, m.z[c] - t.x[c], m.var[c]);
        ++n;
      }
    }
  } else {
    const TrkLink l = links[m.link];
    const TrkNode pt = nodes[l.tx], pr = nodes[l.rx];
    double gx, gy, rsum;
    trk_geom(t, pt, pr, height, gx, gy, rsum);
    {
      const double H[4] = {gx, gy, 0.0, 0.0};
      d2 += trk_component(t, H, m.z[0] - rsum, m.var[0]);
      ++n;
    }
    if (m.z[1] == m.z[1]) {
      const double ex = t.x[0] - pr.x, ey = t.x[1] - pr.y, e2 = ex * ex + ey * ey;
      if (e2 != 0.0) {
        const double w = m.z[1] - atan2(ey, ex) * kTrkRadToDeg;
        const double H[4] = {kTrkRadToDeg * -ey / e2, kTrkRadToDeg * ex / e2, 0.0, 0.0};
        d2 += trk_component(t, H, w - 360.0 * floor((w + 180.0) / 360.0), m.var[1]);
        ++n;
      }
    }
    if (m.z[2] == m.z[2]) {
      trk_geom(t, pt, pr, height, gx, gy, rsum);
      const double H[4] = {0.0, 0.0, -gx, -gy};
      d2 += trk_component(t, H, m.z[2] + (t.x[2] * gx + t.x[3] * gy), m.var[2]);
      ++n;
    }
  }
  *n_comp = n;
  return d2;
}

__device__ __forceinline__ void trk_predict(Trk& t, double dt, double q) {
  t.x[0] += dt * t.x[2];
  t.x[1] += dt * t.x[3];
  double A[16];                                                            // F P
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    A[j] = t.P[j] + dt * t.P[8 + j];
    A[4 + j] = t.P[4 + j] + dt * t.P[12 + j];
    A[8 + j] = t.P[8 + j];
    A[12 + j] = t.P[12 + j];
  }
  const double dt2 = dt * dt, q4 = q * (dt2 * dt2 / 4.0), q3 = q * (dt2 * dt / 2.0), q2 = q * dt2;
#pragma unroll
  for (int i = 0; i < 4; ++i) {                                            // (F P) F^T
    t.P[4 * i] = A[4 * i] + dt * A[4 * i + 2];
    t.P[4 * i + 1] = A[4 * i + 1] + dt * A[4 * i + 3];
    t.P[4 * i + 2] = A[4 * i + 2];
    t.P[4 * i + 3] = A[4 * i + 3];
  }
  t.P[0] += q4; t.P[5] += q4; t.P[2] += q3; t.P[8] += q3; t.P[7] += q3; t.P[13] += q3; t.P[10] += q2; t.P[15] += q2;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = i + 1; j < 4; ++j) { const double m = 0.5 * (t.P[4 * i + j] + t.P[4 * j + i]); t.P[4 * i + j] = m; t.P[4 * j + i] = m; }
}

// flag -> (its rank among the block's flags in thread order, the block's count); s_w [4]; begins with a barrier, ends with one
__device__ __forceinline__ int trk_rank(bool flag, int* s_w, int* total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long b = __ballot(flag);
  __syncthreads();
  if (lane == 0) s_w[wave] = __popcll(b);
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) { before += w < wave ? s_w[w] : 0; all += s_w[w]; }
  *total = all;
  return before + __popcll(b & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(kTrkBlock) void track_step_kernel(TrkState st, TrkPar par, const TrkNode* __restrict__ nodes, const TrkLink* __restrict__ links,
                                                               const TrkMeas* __restrict__ meas, const int* __restrict__ bank_group /* [B + 1] */,
                                                               const TrkGroup* __restrict__ groups, int* __restrict__ assoc, int* __restrict__ assoc_kind,
                                                               int* __restrict__ n_confirmed) {
  __shared__ TrkMeas s_m[ISAC_TRACK_MAX_GROUP_MEAS];
  __shared__ int s_taken[ISAC_TRACK_MAX_GROUP_MEAS];                      // the slot that took the group's measurement i, or -1
  __shared__ int s_birth[ISAC_TRACK_MAX_TRACKS];                          // the bank's unassigned fixes in measurement order, the first 256
  __shared__ int s_free[ISAC_TRACK_MAX_TRACKS];                           // the r-th free slot
  __shared__ double s_rd[4];
  __shared__ int s_rs[4], s_rm[4], s_w[4];
  const int tid = threadIdx.x, bank = blockIdx.x, T = par.T, lane = tid & 63, wave = tid >> 6;
  const bool owns = tid < T;
  const size_t slot = (size_t)bank * T + (owns ? tid : 0);
  Trk t;
  int status = 0, hits = 0, misses = 0, age = 0, id = 0, dof = 0;
  double nis = 0.0;
  if (owns) {
    status = st.status[slot]; id = st.id[slot]; age = st.age[slot]; hits = st.hits[slot]; misses = st.misses[slot];
#pragma unroll
    for (int i = 0; i < 4; ++i) t.x[i] = st.x[4 * slot + i];
#pragma unroll
    for (int i = 0; i < 16; ++i) t.P[i] = st.P[16 * slot + i];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) t.x[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) t.P[i] = 0.0;
  }
  const bool live = owns && status != 0;
  if (live) trk_predict(t, par.dt, par.q);
  bool got_any = false;
  int n_birth = 0;                                                         // (block-uniform) the bank's unassigned fixes so far
  for (int g = bank_group[bank]; g < bank_group[bank + 1]; ++g) {          // (block-uniform throughout)
    const TrkGroup grp = groups[g];
    const int n = grp.end - grp.first;                                     // 1 .. 256
    __syncthreads();                                                       // the group before is done with s_m and s_taken
    if (tid < n) { s_m[tid] = meas[grp.first + tid]; s_taken[tid] = -1; }
    __syncthreads();
    bool in_group = live;                                                  // still without a measurement of this group
    double best_d2 = INFINITY;
    int best_m = -1;
    bool walk = in_group;
    for (;;) {
      if (walk) {
        best_d2 = INFINITY; best_m = -1;
        for (int m = 0; m < n; ++m) {
          if (s_taken[m] >= 0) continue;
          Trk c = t;
          int nc;
          const double d2 = trk_apply(c, s_m[m], nodes, links, par.height, &nc);
          if (d2 <= par.gate2 && d2 < best_d2) { best_d2 = d2; best_m = m; }
        }
      }
      // ---- the block's argmin on (d^2, slot): a thread offers at most one pair, its lowest measurement of the smallest d^2
      double kd = in_group && best_m >= 0 ? best_d2 : INFINITY;
      int ks = in_group && best_m >= 0 ? tid : kTrkBlock, km = best_m;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double od = __shfl_xor(kd, off, 64);
        const int os = __shfl_xor(ks, off, 64), om = __shfl_xor(km, off, 64);
        if (od < kd || (od == kd && os < ks)) { kd = od; ks = os; km = om; }
      }
      if (lane == 0) { s_rd[wave] = kd; s_rs[wave] = ks; s_rm[wave] = km; }
      __syncthreads();
      kd = s_rd[0]; ks = s_rs[0]; km = s_rm[0];
#pragma unroll
      for (int w = 1; w < 4; ++w)
        if (s_rd[w] < kd || (s_rd[w] == kd && s_rs[w] < ks)) { kd = s_rd[w]; ks = s_rs[w]; km = s_rm[w]; }
      if (ks >= kTrkBlock) break;                                          // nobody offers a pair
      if (tid == ks) {
        int nc;
        nis += trk_apply(t, s_m[km], nodes, links, par.height, &nc);
        dof += nc;
        got_any = true;
        in_group = false;
        s_taken[km] = tid;
      }
      walk = in_group && best_m == km;                                     // my best is gone: walk again
      __syncthreads();                                                     // s_taken is seen; s_rd .. may be rewritten
    }
    // ---- the group's measurements: taken ones are final; its unassigned fixes join the bank's list
    const bool mine = tid < n;
    const int taken = mine ? s_taken[tid] : -1;
    const bool unborn = mine && taken < 0 && s_m[tid].kind == 0;
    int n_new;
    const int r = n_birth + trk_rank(unborn, s_w, &n_new);
    if (mine) {
      const int m = grp.first + tid;
      if (!unborn) { assoc[m] = taken; assoc_kind[m] = taken >= 0 ? 1 : 0; }
      else if (r < ISAC_TRACK_MAX_TRACKS) s_birth[r] = m;
      else { assoc[m] = -1; assoc_kind[m] = 3; }                           // behind 256 others: no table has room
    }
    n_birth += n_new;
  }
  // ---- bookkeeping
  if (live) {
    age += 1;
    if (got_any) { hits += 1; misses = 0; } else misses += 1;
    if (status == 1 && hits >= par.confirm_hits) status = 2;
    if ((status == 1 && misses >= par.tent_misses) || (status == 2 && misses >= par.max_misses)) status = 0;
  }
  // ---- births: the r-th free slot takes the r-th unassigned fix
  const bool is_free = owns && status == 0;
  int n_free;
  const int fr = trk_rank(is_free, s_w, &n_free);
  if (is_free) s_free[fr] = tid;
  __syncthreads();                                                         // s_free and every group's s_birth
  const int listed = n_birth < ISAC_TRACK_MAX_TRACKS ? n_birth : ISAC_TRACK_MAX_TRACKS, n_born = listed < n_free ? listed : n_free;
  const int next_id = st.next_id[bank];
  if (tid < listed) {
    const int m = s_birth[tid];
    assoc[m] = tid < n_born ? s_free[tid] : -1;
    assoc_kind[m] = tid < n_born ? 2 : 3;
  }
  if (is_free && fr < n_born) {
    const TrkMeas m = meas[s_birth[fr]];
#pragma unroll
    for (int i = 0; i < 16; ++i) t.P[i] = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const bool have = m.z[c] == m.z[c];
      t.x[c] = have ? m.z[c] : 0.0;
      t.P[5 * c] = have ? m.var[c] : par.v02;
    }
    status = 1; hits = 1; misses = 0; age = 1; nis = 0.0; dof = 0;
    id = next_id + fr + 1;
  }
  const int n_conf = __syncthreads_count(owns && status == 2);             // (also: every thread has read next_id)
  if (tid == 0) { st.next_id[bank] = next_id + n_born; n_confirmed[bank] = n_conf; }
  if (owns) {
    st.status[slot] = status; st.id[slot] = id; st.age[slot] = age; st.hits[slot] = hits; st.misses[slot] = misses; st.dof[slot] = dof; st.nis[slot] = nis;
#pragma unroll
    for (int i = 0; i < 4; ++i) st.x[4 * slot + i] = t.x[i];
#pragma unroll
    for (int i = 0; i < 16; ++i) st.P[16 * slot + i] = t.P[i];
  }
}

// ---------------------------------------------------------------- host side
static bool trk_dims_ok(int B, int T) { return B >= 1 && B <= ISAC_TRACK_MAX_BANKS && T >= 1 && T <= ISAC_TRACK_MAX_TRACKS; }

static int trk_table_args(isac_ctx* ctx, const char* who, const void* d_state, int B, int T, const void* const* outs, int n_outs) {
  if (!d_state) return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": a NULL state block");
  if (!trk_dims_ok(B, T)) return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": 1 <= n_banks <= 1024 and 1 <= max_tracks <= 256 are required");
  for (int i = 0; i < n_outs; ++i)
    if (!outs[i]) return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": a NULL output");
  return ISAC_OK;
}

static int trk_fetch_table(isac_ctx* ctx, const TrkState& s, int B, int T, int32_t* status, int32_t* id, int32_t* age, int32_t* hits, int32_t* misses, double* x, double* P,
                           double* nis, int32_t* dof) {
  const size_t n = (size_t)B * T;
  ISAC_TRY(copy_d2h(ctx, status, s.status, sizeof(int) * n));
  ISAC_TRY(copy_d2h(ctx, id, s.id, sizeof(int) * n));
  ISAC_TRY(copy_d2h(ctx, age, s.age, sizeof(int) * n));
  ISAC_TRY(copy_d2h(ctx, hits, s.hits, sizeof(int) * n));
  ISAC_TRY(copy_d2h(ctx, misses, s.misses, sizeof(int) * n));
  ISAC_TRY(copy_d2h(ctx, x, s.x, sizeof(double) * 4 * n));
  ISAC_TRY(copy_d2h(ctx, P, s.P, sizeof(double) * 16 * n));
  ISAC_TRY(copy_d2h(ctx, nis, s.nis, sizeof(double) * n));
  ISAC_TRY(copy_d2h(ctx, dof, s.dof, sizeof(int) * n));
  return ISAC_OK;
}

}  // namespace isac

using namespace isac;

extern "C" int64_t isac_track_state_bytes(int32_t n_banks, int32_t max_tracks) {
  return trk_dims_ok(n_banks, max_tracks) ? (int64_t)trk_state(nullptr, n_banks, max_tracks).bytes : 0;
}

extern "C" int isac_track_reset_dev(isac_ctx* ctx, void* d_state, int32_t n_banks, int32_t max_tracks) {
  ISAC_TRY(trk_table_args(ctx, "isac_track_reset_dev", d_state, n_banks, max_tracks, nullptr, 0));
  ISAC_ENTER(ctx);
  ISAC_HIP(hipMemsetAsync(d_state, 0, trk_state(nullptr, n_banks, max_tracks).bytes, ctx->stream));
  ISAC_HIP(hipStreamSynchronize(ctx->stream));
  return ISAC_OK;
}

extern "C" int isac_track_get_dev(isac_ctx* ctx, const void* d_state, int32_t n_banks, int32_t max_tracks, int32_t* status, int32_t* id, int32_t* age, int32_t* hits,
                                  int32_t* misses, double* x, double* P, double* nis, int32_t* dof) {
  const void* outs[] = {status, id, age, hits, misses, x, P, nis, dof};
  ISAC_TRY(trk_table_args(ctx, "isac_track_get_dev", d_state, n_banks, max_tracks, outs, 9));
  ISAC_ENTER(ctx);
  return trk_fetch_table(ctx, trk_state(const_cast<void*>(d_state), n_banks, max_tracks), n_banks, max_tracks, status, id, age, hits, misses, x, P, nis, dof);
}

extern "C" int isac_track_step_dev(isac_ctx* ctx, void* d_state, int32_t n_banks, int32_t max_tracks, const double* nodes, int32_t n_nodes, const int32_t* link_tx,
                                   const int32_t* link_rx, int32_t n_links, double height, double dt, double sigma_acc, double gate, int32_t confirm_hits, int32_t tent_misses,
                                   int32_t max_misses, double init_v0, const int32_t* bank_first, const int32_t* meas_group, const int32_t* meas_kind, const int32_t* meas_link,
                                   const double* meas_z, const double* meas_sigma, int32_t* status, int32_t* id, int32_t* age, int32_t* hits, int32_t* misses, double* x,
                                   double* P, double* nis, int32_t* dof, int32_t* assoc, int32_t* assoc_kind, int32_t* n_confirmed) {
  // ---- every check first, on the host alone (they need no device, and a refusal must come before any device work)
  const char* who = "isac_track_step_dev";
  auto bad = [&](const char* what) { return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": " + what); };
  const void* outs[] = {status, id, age, hits, misses, x, P, nis, dof, n_confirmed};
  ISAC_TRY(trk_table_args(ctx, who, d_state, n_banks, max_tracks, outs, 10));
  const int B = n_banks, T = max_tracks, N = n_nodes, K = n_links;
  if (!nodes || !link_tx || !link_rx || !bank_first) return bad("a NULL scene array or bank_first");
  if (N < 1 || N > ISAC_TRACK_MAX_NODES || K < 1 || K > ISAC_TRACK_MAX_LINKS) return bad("1 <= N <= 64 and 1 <= K <= 256 are required");
  if (!std::isfinite(height) || !std::isfinite(dt) || !std::isfinite(sigma_acc) || !std::isfinite(gate) || !std::isfinite(init_v0) || !(dt >= 0.0) || !(sigma_acc >= 0.0))
    return bad("height, dt, sigma_acc, gate and init_v0 finite, dt >= 0 and sigma_acc >= 0 are required");
  if (confirm_hits < 1 || tent_misses < 1 || max_misses < 1) return bad("confirm_hits, tent_misses and max_misses >= 1 are required");
  for (int i = 0; i < 3 * N; ++i)
    if (!std::isfinite(nodes[i])) return bad("a node position that is not finite");
  for (int k = 0; k < K; ++k)
    if (link_tx[k] < 0 || link_tx[k] >= N || link_rx[k] < 0 || link_rx[k] >= N) return bad("a link's node index outside 0 .. N - 1");
  if (bank_first[0] != 0) return bad("bank_first[0] must be 0");
  for (int b = 0; b < B; ++b)
    if (bank_first[b + 1] < bank_first[b] || bank_first[b + 1] > ISAC_TRACK_MAX_MEAS) return bad("bank_first descending or above 2^20");
  const int M = bank_first[B];
  if (M > 0 && (!meas_group || !meas_kind || !meas_link || !meas_z || !meas_sigma || !assoc || !assoc_kind)) return bad("a NULL measurement array, assoc or assoc_kind");
  std::vector<int> bank_group(B + 1, 0);
  std::vector<TrkGroup> groups;
  for (int b = 0; b < B; ++b) {
    for (int m = bank_first[b]; m < bank_first[b + 1]; ++m) {
      const bool first = m == bank_first[b];
      if (meas_group[m] < 0 || meas_group[m] >= ISAC_TRACK_MAX_GROUPS || (!first && meas_group[m] < meas_group[m - 1])) return bad("meas_group outside 0 .. 255 or not ascending inside a bank");
      if (meas_kind[m] != 0 && meas_kind[m] != 1) return bad("meas_kind must be 0 or 1");
      if (meas_kind[m] == 1 && (meas_link[m] < 0 || meas_link[m] >= K)) return bad("the link of a kind-1 measurement outside 0 .. K - 1");
      const double* z = meas_z + 4 * (size_t)m;
      for (int c = 0; c < 4; ++c) {
        const double s = meas_sigma[4 * (size_t)m + c];
        if (!std::isfinite(s) || !(s > 0.0)) return bad("a sigma that is not finite and > 0");
      }
      if (meas_kind[m] == 0 ? !std::isfinite(z[0]) || !std::isfinite(z[1]) || std::isinf(z[2]) || std::isinf(z[3]) : !std::isfinite(z[0]) || std::isinf(z[1]) || std::isinf(z[2]))
        return bad("a measured value that is not finite (or NaN where NaN means absent)");
      if (first || meas_group[m] != meas_group[m - 1]) groups.push_back(TrkGroup{m, m + 1});
      else if (++groups.back().end - groups.back().first > ISAC_TRACK_MAX_GROUP_MEAS) return bad("more than 256 measurements in a group");
    }
    bank_group[b + 1] = (int)groups.size();
  }
  ISAC_ENTER(ctx);
  // ---- one staged upload: nodes | links | bank_group | groups | measurements
  std::vector<TrkNode> nd(N);
  for (int n = 0; n < N; ++n) nd[n] = TrkNode{nodes[3 * n], nodes[3 * n + 1], nodes[3 * n + 2]};
  std::vector<TrkLink> lk(K);
  for (int k = 0; k < K; ++k) lk[k] = TrkLink{link_tx[k], link_rx[k]};
  Carver cv;
  const size_t off_nd = cv.take(sizeof(TrkNode) * N), off_lk = cv.take(sizeof(TrkLink) * K), off_bg = cv.take(sizeof(int) * (B + 1));
  const size_t off_gr = cv.take(sizeof(TrkGroup) * groups.size()), off_ms = cv.take(sizeof(TrkMeas) * (size_t)M), up_bytes = (cv.total + 15) & ~(size_t)15;
  const size_t off_as = cv.take(sizeof(int) * (size_t)M), off_ak = cv.take(sizeof(int) * (size_t)M), off_nc = cv.take(sizeof(int) * B);
  ISAC_TRY(ensure(ctx, ctx->track, cv.total + 16));
  char* d = (char*)ctx->track.p;
  void* h = nullptr;
  ISAC_TRY(stage_acquire(ctx, up_bytes, &h));
  std::memset(h, 0, up_bytes);
  std::memcpy((char*)h + off_nd, nd.data(), sizeof(TrkNode) * N);
  std::memcpy((char*)h + off_lk, lk.data(), sizeof(TrkLink) * K);
  std::memcpy((char*)h + off_bg, bank_group.data(), sizeof(int) * (B + 1));
  if (!groups.empty()) std::memcpy((char*)h + off_gr, groups.data(), sizeof(TrkGroup) * groups.size());
  TrkMeas* hm = (TrkMeas*)((char*)h + off_ms);
  for (int m = 0; m < M; ++m) {
    TrkMeas& r = hm[m];
    for (int c = 0; c < 4; ++c) { r.z[c] = meas_z[4 * (size_t)m + c]; r.var[c] = meas_sigma[4 * (size_t)m + c] * meas_sigma[4 * (size_t)m + c]; }
    r.kind = meas_kind[m];
    r.link = r.kind == 1 ? meas_link[m] : 0;
  }
  ISAC_TRY(stage_commit(ctx, d, up_bytes));
  const TrkState st = trk_state(d_state, B, T);
  const TrkPar par{dt, sigma_acc * sigma_acc, gate * gate, init_v0 * init_v0, height, confirm_hits, tent_misses, max_misses, T};
  ISAC_TRY(profile_begin(ctx));
  hipLaunchKernelGGL(track_step_kernel, dim3(B), dim3(kTrkBlock), 0, ctx->stream, st, par, (const TrkNode*)(d + off_nd), (const TrkLink*)(d + off_lk),
                     (const TrkMeas*)(d + off_ms), (const int*)(d + off_bg), (const TrkGroup*)(d + off_gr), (int*)(d + off_as), (int*)(d + off_ak), (int*)(d + off_nc));
  ISAC_TRY(profile_end(ctx));
  ISAC_HIP(hipGetLastError());
  ISAC_TRY(trk_fetch_table(ctx, st, B, T, status, id, age, hits, misses, x, P, nis, dof));
  ISAC_TRY(copy_d2h(ctx, assoc, d + off_as, sizeof(int) * (size_t)M));
  ISAC_TRY(copy_d2h(ctx, assoc_kind, d + off_ak, sizeof(int) * (size_t)M));
  ISAC_TRY(copy_d2h(ctx, n_confirmed, d + off_nc, sizeof(int) * B));
  return ISAC_OK;
}
