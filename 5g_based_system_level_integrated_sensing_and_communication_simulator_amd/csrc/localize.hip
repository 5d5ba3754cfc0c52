// Multi-static localisation (gfx950 only): isac_position_map_dev and isac_localize_dev (include/isac_localize.h has the definition; project-defined).
//   A  position_map_kernel   S(g) = sum_links exp(-min_{m in link} q_m(g) / 2) on the grid                     the hot path
//   B  peak_kernel           the candidates of a block's stretch of the map, its best max_cand by (value descending, flat index ascending)
//      peak_merge_kernel     the blocks' lists into one, the same order                                         one workgroup
//   C  greedy_kernel         associate / refine / claim, candidate after candidate                              one workgroup
// position_map_kernel: one thread per grid point, 64 threads (one wave) a block.  A thread forms its distance to every node ONCE (N square roots) and its azimuth seen
// from a node once, and only for the nodes that receive a measurement with a finite azimuth (a wave-uniform branch on the node table); both go into the thread's own
// column of LDS, [2 N][64] doubles, lane-contiguous (no bank conflict), read back per LINK: two distances and one azimuth.  Nobody else reads a thread's column, so the
// kernel has no barrier.  The tables (nodes, links, the links' first measurement, the measurements as {r, azi, 1 / sigma_r, 1 / sigma_a}) are indexed by loop counters
// only -- wave-uniform addresses, which the compiler turns into scalar loads through the constant cache; a measurement costs the vector units ten fp64 operations and
// no transcendental: exp is monotone, so the link's maximum of exp(-q / 2) is exp(-min q / 2), one exponential per (point, link).  A NaN azimuth is stored as azi = 0 with
// 1 / sigma_a = 0: its term is exactly +0 and the loop has no branch.  The links are summed ascending by the owning thread: no reduction, no atomics, the same bits on every
// run and for any block shape.  A column of N <= 64 nodes is at most 64 KB of LDS a block (N KB): two blocks a CU at N = 64, seven at N = 21.
// peak_kernel / peak_merge_kernel keep a sorted best list in LDS and push tiles of 256 entries through one bitonic sort of 512: the top max_cand of a strict total order is
// one set whatever the order of arrival, and the lists are written sorted.  No atomics.
// greedy_kernel: 256 threads.  q of every measurement at the cell centre in parallel over measurements; one thread per link picks; the Gauss-Newton and velocity terms are
// formed by one thread per link into LDS and summed by EVERY thread in ascending link order (refine_eval's idiom: all threads hold the same bits and take the same branch).
#include <cmath>
#include <vector>

#include "isac_internal.hpp"
#include "cpi_post.hpp"
#include "../../include/isac_localize.h"

namespace isac {

constexpr int kMapBlock = 64;
constexpr int kPeakBlocks = 512;                                          // at most: each takes a contiguous stretch of the map
constexpr double kRadToDeg = 57.29577951308232087679815481410517;
constexpr double kSingular = 1e-12, kVelCond = 1e-8;

struct LocNode { double x, y, z, wants_azi; };                            // wants_azi != 0: some measurement received here has a finite azimuth
struct LocLink { int tx, rx, first, end; };                               // measurements first .. end - 1
struct LocMeas { double r, azi, inv_sr, inv_sa; };                        // a NaN azimuth: azi = 0, inv_sa = 0
struct LocGrid { double x0, dx, y0, dy, z; int nx, ny; };
struct LocCand { double s; int cell; int pad; };                          // cell < 0: an empty slot, behind every real one

__device__ __forceinline__ double wrap_deg(double d) { return d - 360.0 * floor((d + 180.0) * (1.0 / 360.0)); }
__device__ __forceinline__ double azimuth_deg(double ey, double ex) { return atan2(ey, ex) * kRadToDeg; }

__global__ __launch_bounds__(kMapBlock) void position_map_kernel(const LocNode* __restrict__ nodes, int N, const LocLink* __restrict__ links, int K,
                                                                 const LocMeas* __restrict__ meas, LocGrid g, double* __restrict__ map) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* s_d = reinterpret_cast<double*>(smem_raw) + threadIdx.x;        // [N][64] distances, then [N][64] azimuths: this thread's column
  double* s_a = s_d + N * kMapBlock;
  const long long cell = (long long)blockIdx.x * kMapBlock + threadIdx.x;
  if (cell >= (long long)g.nx * g.ny) return;
  const int iy = (int)(cell / g.nx), ix = (int)(cell - (long long)iy * g.nx);
  const double x = g.x0 + (double)ix * g.dx, y = g.y0 + (double)iy * g.dy;
  for (int n = 0; n < N; ++n) {
    const double ex = x - nodes[n].x, ey = y - nodes[n].y, ez = g.z - nodes[n].z;
    s_d[n * kMapBlock] = sqrt(ex * ex + ey * ey + ez * ez);
    s_a[n * kMapBlock] = nodes[n].wants_azi != 0.0 ? azimuth_deg(ey, ex) : 0.0;   // (wave-uniform)
  }
  double S = 0.0;
  for (int k = 0; k < K; ++k) {
    const LocLink l = links[k];
    const double dsum = s_d[l.tx * kMapBlock] + s_d[l.rx * kMapBlock], az = s_a[l.rx * kMapBlock];
    double qmin = INFINITY;                                                // a link without a measurement: exp(-inf) = 0
    for (int m = l.first; m < l.end; ++m) {
      const LocMeas t = meas[m];
      const double a = (dsum - t.r) * t.inv_sr, b = wrap_deg(az - t.azi) * t.inv_sa;
      const double q = a * a + b * b;
      qmin = q < qmin ? q : qmin;
    }
    S += exp(-0.5 * qmin);
  }
  map[cell] = S;
}

// ---------------------------------------------------------------- B
__device__ __forceinline__ bool cand_before(const LocCand& a, const LocCand& b) {
  if (a.cell < 0 || b.cell < 0) return a.cell >= 0 && b.cell < 0;
  return a.s > b.s || (a.s == b.s && a.cell < b.cell);
}

// s_c [512], 256 threads: sorted so that cand_before holds along the array.  Begins and ends with a barrier.
__device__ __forceinline__ void cand_sort512(LocCand* s_c) {
  const int tid = threadIdx.x;
  for (int k = 2; k <= 512; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      const int i = ((tid & ~(j - 1)) << 1) | (tid & (j - 1)), p = i | j;  // the pair (i, i + j), i without bit j
      const bool up = (i & k) == 0;
      const LocCand a = s_c[i], b = s_c[p];
      if (up ? cand_before(b, a) : cand_before(a, b)) { s_c[i] = b; s_c[p] = a; }
    }
  __syncthreads();
}

__device__ __forceinline__ bool is_candidate(const double* __restrict__ map, int nx, int ny, long long cell, double min_score) {
  const double s = map[cell];
  if (!(s >= min_score)) return false;
  const int iy = (int)(cell / nx), ix = (int)(cell - (long long)iy * nx);
  bool ok = true;
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      const int jx = ix + dx, jy = iy + dy;
      if ((dx == 0 && dy == 0) || jx < 0 || jx >= nx || jy < 0 || jy >= ny) continue;
      const double v = map[(long long)jy * nx + jx];
      ok = ok && (dy < 0 || (dy == 0 && dx < 0) ? s > v : s >= v);
    }
  return ok;
}

// The best `keep` (<= 256) of s_c[0 .. 255] (sorted, the list so far) and s_c[256 .. 511] (a tile) into s_c[0 .. 255].  `any`: the tile holds an entry (block-uniform).
__device__ __forceinline__ void cand_push(LocCand* s_c, int keep, bool any) {
  if (!any) return;
  cand_sort512(s_c);
  if ((int)threadIdx.x >= keep) s_c[threadIdx.x].cell = -1;
  __syncthreads();
}

__global__ __launch_bounds__(256) void peak_kernel(const double* __restrict__ map, int nx, int ny, double min_score, int keep, long long per_block,
                                                   LocCand* __restrict__ part /* [blocks][256] */) {
  __shared__ LocCand s_c[512];
  const int tid = threadIdx.x;
  const long long total = (long long)nx * ny, lo = (long long)blockIdx.x * per_block, hi = lo + per_block < total ? lo + per_block : total;
  s_c[tid].cell = -1;
  for (long long c0 = lo; c0 < hi; c0 += 256) {                            // (block-uniform)
    const long long cell = c0 + tid;
    const bool c = cell < hi && is_candidate(map, nx, ny, cell, min_score);
    s_c[256 + tid] = LocCand{c ? map[cell] : 0.0, c ? (int)cell : -1, 0};
    cand_push(s_c, keep, __syncthreads_or(c) != 0);
  }
  __syncthreads();
  part[(long long)blockIdx.x * 256 + tid] = s_c[tid];
}

__global__ __launch_bounds__(256) void peak_merge_kernel(const LocCand* __restrict__ part, int blocks, int keep, LocCand* __restrict__ cand /* [256] */, int* __restrict__ n_cand) {
  __shared__ LocCand s_c[512];
  const int tid = threadIdx.x;
  s_c[tid].cell = -1;
  for (int b = 0; b < blocks; ++b) {
    const LocCand c = part[(long long)b * 256 + tid];
    s_c[256 + tid] = c;
    cand_push(s_c, keep, __syncthreads_or(c.cell >= 0) != 0);
  }
  __syncthreads();
  cand[tid] = s_c[tid];
  const int n = __syncthreads_count(s_c[tid].cell >= 0);
  if (tid == 0) *n_cand = n;
}

// ---------------------------------------------------------------- C
struct LocOut {                                                           // device pointers of the outputs' copies
  double* pos; double* vel; int* vel_status; double* score; int* n_links; int* assoc; double* rms; int* cand_cell; double* cand_score; int* cand_status; int* n_out;
};
struct LocPar { double gate2, max_move; int min_links, iters, max_targets; };

struct LocGeom { double rho, alpha, jx, jy, ax, ay; };                    // rho and its gradient (u_tx + u_rx)_xy; alpha and its gradient

__device__ __forceinline__ LocGeom loc_geom(const LocNode& pt, const LocNode& pr, double x, double y, double z, double r, double azi, bool use_azi) {
  const double tx = x - pt.x, ty = y - pt.y, tz = z - pt.z, rx = x - pr.x, ry = y - pr.y, rz = z - pr.z;
  const double dt = sqrt(tx * tx + ty * ty + tz * tz), dr = sqrt(rx * rx + ry * ry + rz * rz);
  LocGeom o;
  o.rho = (dt + dr) - r;
  o.jx = tx / dt + rx / dr;
  o.jy = ty / dt + ry / dr;
  o.alpha = 0.0; o.ax = 0.0; o.ay = 0.0;
  if (use_azi) {
    const double h2 = rx * rx + ry * ry;
    o.alpha = wrap_deg(azimuth_deg(ry, rx) - azi);
    o.ax = -kRadToDeg * ry / h2;
    o.ay = kRadToDeg * rx / h2;
  }
  return o;
}

__global__ __launch_bounds__(256) void greedy_kernel(const LocNode* __restrict__ nodes, const LocLink* __restrict__ links, int K, const LocMeas* __restrict__ meas,
                                                     const double* __restrict__ meas_s, const double* __restrict__ inv_sv, int M, LocGrid g,
                                                     const LocCand* __restrict__ cand, const int* __restrict__ n_cand_p, LocPar par, LocOut out) {
  __shared__ double s_q[ISAC_LOCALIZE_MAX_MEAS];
  __shared__ unsigned char s_claimed[ISAC_LOCALIZE_MAX_MEAS];
  __shared__ int s_assoc[ISAC_LOCALIZE_MAX_LINKS];
  __shared__ double s_t[6][ISAC_LOCALIZE_MAX_LINKS];                      // a link's terms of the sums
  const int tid = threadIdx.x, n_cand = *n_cand_p;
  for (int m = tid; m < M; m += 256) s_claimed[m] = 0;
  int n_acc = 0;
  auto q_at = [&](int k, int m, double x, double y) {                     // q of measurement m (of link k) at (x, y)
    const LocMeas t = meas[m];
    const LocGeom e = loc_geom(nodes[links[k].tx], nodes[links[k].rx], x, y, g.z, t.r, t.azi, t.inv_sa != 0.0);
    const double a = e.rho * t.inv_sr, b = e.alpha * t.inv_sa;
    return a * a + b * b;
  };
  for (int c = 0; c < n_cand; ++c) {                                      // (block-uniform throughout)
    const int cell = cand[c].cell, iy = cell / g.nx, ix = cell - iy * g.nx;
    const double xc = g.x0 + (double)ix * g.dx, yc = g.y0 + (double)iy * g.dy;
    __syncthreads();
    // ---- 1: q at the cell centre, every measurement; then a thread per link
    for (int k = 0; k < K; ++k)
      for (int m = links[k].first + tid; m < links[k].end; m += 256) s_q[m] = q_at(k, m, xc, yc);
    __syncthreads();
    if (tid < K) {
      int best = -1;
      double qb = 0.0;
      for (int m = links[tid].first; m < links[tid].end; ++m)
        if (!s_claimed[m] && (best < 0 || s_q[m] < qb)) { best = m; qb = s_q[m]; }
      s_assoc[tid] = best >= 0 && qb <= par.gate2 ? best : -1;
    }
    __syncthreads();
    int n_l = 0;
    for (int k = 0; k < K; ++k) n_l += s_assoc[k] >= 0;
    int status = n_l < par.min_links ? 1 : 0;
    // ---- 3-4: Gauss-Newton on (x, y), the associated set fixed
    double x = xc, y = yc;
    for (int it = 0; it < par.iters && status == 0; ++it) {
      __syncthreads();
      if (tid < K) {
        double h11 = 0.0, h12 = 0.0, h22 = 0.0, b1 = 0.0, b2 = 0.0;
        const int m = s_assoc[tid];
        if (m >= 0) {
          const LocMeas t = meas[m];
          const LocGeom e = loc_geom(nodes[links[tid].tx], nodes[links[tid].rx], x, y, g.z, t.r, t.azi, t.inv_sa != 0.0);
          const double jx = e.jx * t.inv_sr, jy = e.jy * t.inv_sr, res = e.rho * t.inv_sr;
          const double ax = e.ax * t.inv_sa, ay = e.ay * t.inv_sa, ra = e.alpha * t.inv_sa;
          h11 = jx * jx + ax * ax; h12 = jx * jy + ax * ay; h22 = jy * jy + ay * ay;
          b1 = jx * res + ax * ra; b2 = jy * res + ay * ra;
        }
        s_t[0][tid] = h11; s_t[1][tid] = h12; s_t[2][tid] = h22; s_t[3][tid] = b1; s_t[4][tid] = b2;
      }
      __syncthreads();
      double h11 = 0.0, h12 = 0.0, h22 = 0.0, b1 = 0.0, b2 = 0.0;
      for (int k = 0; k < K; ++k) { h11 += s_t[0][k]; h12 += s_t[1][k]; h22 += s_t[2][k]; b1 += s_t[3][k]; b2 += s_t[4][k]; }
      const double det = h11 * h22 - h12 * h12, ht = 0.5 * (h11 + h22);
      if (!(det > kSingular * ht * ht)) { status = 2; break; }
      x -= (h22 * b1 - h12 * b2) / det;
      y -= (h11 * b2 - h12 * b1) / det;
    }
    if (status == 0) {
      const double mx = x - xc, my = y - yc;
      if (!(sqrt(mx * mx + my * my) <= par.max_move)) status = 3;
    }
    if (status == 0 && n_acc >= par.max_targets) status = 4;
    if (status == 0) {
      // ---- rms and 6: velocity at the final point
      __syncthreads();
      if (tid < K) {
        double q = 0.0, n11 = 0.0, n12 = 0.0, n22 = 0.0, r1 = 0.0, r2 = 0.0, cnt = 0.0;
        const int m = s_assoc[tid];
        if (m >= 0) {
          const LocMeas t = meas[m];
          const LocGeom e = loc_geom(nodes[links[tid].tx], nodes[links[tid].rx], x, y, g.z, t.r, t.azi, t.inv_sa != 0.0);
          const double a = e.rho * t.inv_sr, b = e.alpha * t.inv_sa;
          q = a * a + b * b;
          const double s = meas_s[m];
          if (s == s) {                                                    // not NaN
            const double ax = -e.jx * inv_sv[m], ay = -e.jy * inv_sv[m], ys = s * inv_sv[m];
            n11 = ax * ax; n12 = ax * ay; n22 = ay * ay; r1 = ax * ys; r2 = ay * ys; cnt = 1.0;
          }
        }
        s_t[0][tid] = n11; s_t[1][tid] = n12; s_t[2][tid] = n22; s_t[3][tid] = r1; s_t[4][tid] = r2; s_t[5][tid] = q;
        s_q[tid] = cnt;                                                    // (s_q is rewritten at the next candidate)
      }
      __syncthreads();
      if (tid == 0) {
        double n11 = 0.0, n12 = 0.0, n22 = 0.0, r1 = 0.0, r2 = 0.0, qs = 0.0;
        int cnt = 0;
        for (int k = 0; k < K; ++k) { n11 += s_t[0][k]; n12 += s_t[1][k]; n22 += s_t[2][k]; r1 += s_t[3][k]; r2 += s_t[4][k]; qs += s_t[5][k]; cnt += s_q[k] != 0.0; }
        const double h = 0.5 * (n11 + n22), hd = 0.5 * (n11 - n22), dl = sqrt(hd * hd + n12 * n12), det = n11 * n22 - n12 * n12;
        const bool ok = cnt >= 2 && (h - dl) / (h + dl) >= kVelCond;
        out.pos[2 * n_acc] = x; out.pos[2 * n_acc + 1] = y;
        out.vel[2 * n_acc] = ok ? (n22 * r1 - n12 * r2) / det : NAN;
        out.vel[2 * n_acc + 1] = ok ? (n11 * r2 - n12 * r1) / det : NAN;
        out.vel_status[n_acc] = ok ? 0 : 1;
        out.score[n_acc] = cand[c].s;
        out.n_links[n_acc] = n_l;
        out.rms[n_acc] = sqrt(qs / (double)n_l);
      }
      if (tid < K) {
        out.assoc[(long long)K * n_acc + tid] = s_assoc[tid];
        if (s_assoc[tid] >= 0) s_claimed[s_assoc[tid]] = 1;
      }
      ++n_acc;
    }
    if (tid == 0) { out.cand_cell[c] = cell; out.cand_score[c] = cand[c].s; out.cand_status[c] = status; }
  }
  if (tid == 0) { out.n_out[0] = n_acc; out.n_out[1] = n_cand; }
}

// ---------------------------------------------------------------- host side
struct LocScene {                                                         // the validated scene, packed for one staged upload
  std::vector<LocNode> nodes; std::vector<LocLink> links; std::vector<LocMeas> meas; std::vector<double> s, inv_sv;
  LocGrid grid;
};

static int loc_scene(isac_ctx* ctx, const char* who, const double* nodes, int N, const int32_t* link_tx, const int32_t* link_rx, int K, const int32_t* meas_link,
                     const double* meas_r, const double* meas_s, const double* meas_azi, const double* sigma_r, const double* sigma_v, const double* sigma_a, int M, double x0,
                     double dx, int nx, double y0, double dy, int ny, double z, const void* d_map, LocScene& sc) {
  auto bad = [&](const char* what) { return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": " + what); };
  if (!nodes || !link_tx || !link_rx || !meas_link || !meas_r || !meas_s || !meas_azi || !sigma_r || !sigma_v || !sigma_a || !d_map) return bad("a NULL scene array or map");
  if (N < 1 || N > ISAC_LOCALIZE_MAX_NODES || K < 1 || K > ISAC_LOCALIZE_MAX_LINKS || M < 1 || M > ISAC_LOCALIZE_MAX_MEAS)
    return bad("1 <= N <= 64, 1 <= K <= 256 and 1 <= M <= 4096 are required");
  if (nx < 1 || ny < 1 || nx > ISAC_LOCALIZE_MAX_SIDE || ny > ISAC_LOCALIZE_MAX_SIDE || (long long)nx * ny > ISAC_LOCALIZE_MAX_CELLS)
    return bad("1 <= nx, ny <= 8192 and nx ny <= 2^26 are required");
  if (!std::isfinite(x0) || !std::isfinite(y0) || !std::isfinite(z) || !std::isfinite(dx) || !std::isfinite(dy) || !(dx > 0.0) || !(dy > 0.0))
    return bad("x0, y0, z finite and dx, dy finite and > 0 are required");
  for (int i = 0; i < 3 * N; ++i)
    if (!std::isfinite(nodes[i])) return bad("a node position that is not finite");
  for (int k = 0; k < K; ++k)
    if (link_tx[k] < 0 || link_tx[k] >= N || link_rx[k] < 0 || link_rx[k] >= N) return bad("a link's node index outside 0 .. N - 1");
  for (int m = 0; m < M; ++m) {
    if (meas_link[m] < 0 || meas_link[m] >= K || (m > 0 && meas_link[m] < meas_link[m - 1])) return bad("meas_link outside 0 .. K - 1 or not ascending");
    if (!std::isfinite(meas_r[m])) return bad("a range sum that is not finite");
    for (const double s : {sigma_r[m], sigma_v[m], sigma_a[m]})
      if (!std::isfinite(s) || !(s > 0.0)) return bad("a sigma that is not finite and > 0");
    if (std::isinf(meas_azi[m])) return bad("an azimuth that is infinite");
  }
  sc.grid = LocGrid{x0, dx, y0, dy, z, nx, ny};
  sc.nodes.assign(N, LocNode{0.0, 0.0, 0.0, 0.0});
  for (int n = 0; n < N; ++n) { sc.nodes[n].x = nodes[3 * n]; sc.nodes[n].y = nodes[3 * n + 1]; sc.nodes[n].z = nodes[3 * n + 2]; }
  sc.links.assign(K, LocLink{0, 0, 0, 0});
  sc.meas.resize(M); sc.s.resize(M); sc.inv_sv.resize(M);
  std::vector<int> first(K + 1, 0);                                         // ascending meas_link: link k holds first[k] .. first[k + 1] - 1
  for (int m = 0; m < M; ++m) ++first[meas_link[m] + 1];
  for (int k = 0; k < K; ++k) {
    first[k + 1] += first[k];
    sc.links[k] = LocLink{link_tx[k], link_rx[k], first[k], first[k + 1]};
  }
  for (int m = 0; m < M; ++m) {
    const bool az = !std::isnan(meas_azi[m]);
    sc.meas[m] = LocMeas{meas_r[m], az ? meas_azi[m] : 0.0, 1.0 / sigma_r[m], az ? 1.0 / sigma_a[m] : 0.0};
    if (az) sc.nodes[link_rx[meas_link[m]]].wants_azi = 1.0;
    sc.s[m] = meas_s[m];
    sc.inv_sv[m] = 1.0 / sigma_v[m];
  }
  return ISAC_OK;
}

struct LocTables { size_t nodes, links, meas, s, inv_sv, bytes; };         // offsets in the scene block

static LocTables loc_pack(const LocScene& sc, std::vector<char>& host) {
  Carver cv;
  LocTables t;
  t.nodes = cv.take(sizeof(LocNode) * sc.nodes.size()); t.links = cv.take(sizeof(LocLink) * sc.links.size()); t.meas = cv.take(sizeof(LocMeas) * sc.meas.size());
  t.s = cv.take(sizeof(double) * sc.s.size()); t.inv_sv = cv.take(sizeof(double) * sc.inv_sv.size());
  t.bytes = (cv.total + 15) & ~(size_t)15;
  host.assign(t.bytes, 0);
  std::memcpy(host.data() + t.nodes, sc.nodes.data(), sizeof(LocNode) * sc.nodes.size());
  std::memcpy(host.data() + t.links, sc.links.data(), sizeof(LocLink) * sc.links.size());
  std::memcpy(host.data() + t.meas, sc.meas.data(), sizeof(LocMeas) * sc.meas.size());
  std::memcpy(host.data() + t.s, sc.s.data(), sizeof(double) * sc.s.size());
  std::memcpy(host.data() + t.inv_sv, sc.inv_sv.data(), sizeof(double) * sc.inv_sv.size());
  return t;
}

}  // namespace isac

using namespace isac;

extern "C" int isac_position_map_dev(isac_ctx* ctx, const double* nodes, int32_t n_nodes, const int32_t* link_tx, const int32_t* link_rx, int32_t n_links,
                                     const int32_t* meas_link, const double* meas_r, const double* meas_s, const double* meas_azi, const double* sigma_r, const double* sigma_v,
                                     const double* sigma_a, int32_t n_meas, double x0, double dx, int32_t nx, double y0, double dy, int32_t ny, double z, double* d_map) {
  ISAC_ENTER(ctx);
  LocScene sc;
  ISAC_TRY(loc_scene(ctx, "isac_position_map_dev", nodes, n_nodes, link_tx, link_rx, n_links, meas_link, meas_r, meas_s, meas_azi, sigma_r, sigma_v, sigma_a, n_meas, x0, dx, nx,
                     y0, dy, ny, z, d_map, sc));
  std::vector<char> host;
  const LocTables t = loc_pack(sc, host);
  ISAC_TRY(ensure(ctx, ctx->localize, t.bytes));
  char* d = (char*)ctx->localize.p;
  ISAC_TRY(stage_upload(ctx, d, host.data(), t.bytes));
  const size_t lds = sizeof(double) * 2 * (size_t)n_nodes * kMapBlock;      // <= 64 KB at N = 64
  ISAC_TRY(profile_begin(ctx));
  hipLaunchKernelGGL(position_map_kernel, dim3(cdiv((long long)nx * ny, kMapBlock)), dim3(kMapBlock), lds, ctx->stream, (const LocNode*)(d + t.nodes), n_nodes,
                     (const LocLink*)(d + t.links), n_links, (const LocMeas*)(d + t.meas), sc.grid, d_map);
  ISAC_TRY(profile_end(ctx));
  ISAC_HIP(hipGetLastError());
  ISAC_HIP(hipStreamSynchronize(ctx->stream));
  return ISAC_OK;
}

extern "C" int isac_localize_dev(isac_ctx* ctx, const double* nodes, int32_t n_nodes, const int32_t* link_tx, const int32_t* link_rx, int32_t n_links,
                                 const int32_t* meas_link, const double* meas_r, const double* meas_s, const double* meas_azi, const double* sigma_r, const double* sigma_v,
                                 const double* sigma_a, int32_t n_meas, double x0, double dx, int32_t nx, double y0, double dy, int32_t ny, double z, const double* d_map,
                                 double min_score, int32_t max_cand, int32_t min_links, double gate, int32_t iters, double max_move, int32_t max_targets, double* pos,
                                 double* vel, int32_t* vel_status, double* score, int32_t* n_links_out, int32_t* assoc, double* rms, int32_t* cand_cell, double* cand_score,
                                 int32_t* cand_status, int32_t* n_out) {
  ISAC_ENTER(ctx);
  const char* who = "isac_localize_dev";
  LocScene sc;
  ISAC_TRY(loc_scene(ctx, who, nodes, n_nodes, link_tx, link_rx, n_links, meas_link, meas_r, meas_s, meas_azi, sigma_r, sigma_v, sigma_a, n_meas, x0, dx, nx, y0, dy, ny, z,
                     d_map, sc));
  if (max_cand < 1 || max_cand > ISAC_LOCALIZE_MAX_CAND || max_targets < 1 || max_targets > ISAC_LOCALIZE_MAX_CAND || iters < 0 || iters > ISAC_LOCALIZE_MAX_ITERS || min_links < 0)
    return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": 1 <= max_cand, max_targets <= 256, 0 <= iters <= 64 and min_links >= 0 are required");
  if (!std::isfinite(min_score) || !std::isfinite(gate) || !std::isfinite(max_move))
    return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": min_score, gate and max_move must be finite");
  if (!pos || !vel || !vel_status || !score || !n_links_out || !assoc || !rms || !n_out) return fail(ctx, ISAC_ERR_INVALID_ARG, std::string(who) + ": a NULL output");
  const int K = n_links, T = max_targets, C = ISAC_LOCALIZE_MAX_CAND;
  const long long total = (long long)nx * ny;
  const int blocks = (int)std::min<long long>(kPeakBlocks, cdiv(total, 256));
  const long long per_block = (total + blocks - 1) / blocks;
  std::vector<char> host;
  const LocTables t = loc_pack(sc, host);
  Carver cv;
  cv.take(t.bytes);
  const size_t off_part = cv.take(sizeof(LocCand) * 256 * (size_t)blocks), off_cand = cv.take(sizeof(LocCand) * 256), off_pos = cv.take(sizeof(double) * 2 * T);
  const size_t off_vel = cv.take(sizeof(double) * 2 * T), off_score = cv.take(sizeof(double) * T), off_rms = cv.take(sizeof(double) * T);
  const size_t off_cs = cv.take(sizeof(double) * C), off_vs = cv.take(sizeof(int) * T), off_nl = cv.take(sizeof(int) * T), off_as = cv.take(sizeof(int) * (size_t)K * T);
  const size_t off_cc = cv.take(sizeof(int) * C), off_ct = cv.take(sizeof(int) * C), off_n = cv.take(sizeof(int) * 4);
  ISAC_TRY(ensure(ctx, ctx->localize, cv.total));
  char* d = (char*)ctx->localize.p;
  ISAC_TRY(stage_upload(ctx, d, host.data(), t.bytes));
  hipLaunchKernelGGL(peak_kernel, dim3(blocks), dim3(256), 0, ctx->stream, d_map, nx, ny, min_score, max_cand, per_block, (LocCand*)(d + off_part));
  hipLaunchKernelGGL(peak_merge_kernel, dim3(1), dim3(256), 0, ctx->stream, (const LocCand*)(d + off_part), blocks, max_cand, (LocCand*)(d + off_cand), (int*)(d + off_n) + 2);
  const LocOut out{(double*)(d + off_pos), (double*)(d + off_vel), (int*)(d + off_vs), (double*)(d + off_score), (int*)(d + off_nl), (int*)(d + off_as), (double*)(d + off_rms),
                   (int*)(d + off_cc), (double*)(d + off_cs), (int*)(d + off_ct), (int*)(d + off_n)};
  hipLaunchKernelGGL(greedy_kernel, dim3(1), dim3(256), 0, ctx->stream, (const LocNode*)(d + t.nodes), (const LocLink*)(d + t.links), K, (const LocMeas*)(d + t.meas),
                     (const double*)(d + t.s), (const double*)(d + t.inv_sv), n_meas, sc.grid, (const LocCand*)(d + off_cand), (const int*)(d + off_n) + 2,
                     LocPar{gate * gate, max_move, min_links, iters, max_targets}, out);
  ISAC_HIP(hipGetLastError());
  int n[2] = {0, 0};
  ISAC_TRY(copy_d2h(ctx, n, d + off_n, sizeof(n)));
  if (n[0] < 0 || n[0] > T || n[1] < 0 || n[1] > max_cand) return fail(ctx, ISAC_ERR_HIP, std::string(who) + ": the device returned counts outside their limits");
  const size_t nt = (size_t)n[0], nc = (size_t)n[1];
  ISAC_TRY(copy_d2h(ctx, pos, d + off_pos, sizeof(double) * 2 * nt));
  ISAC_TRY(copy_d2h(ctx, vel, d + off_vel, sizeof(double) * 2 * nt));
  ISAC_TRY(copy_d2h(ctx, vel_status, d + off_vs, sizeof(int) * nt));
  ISAC_TRY(copy_d2h(ctx, score, d + off_score, sizeof(double) * nt));
  ISAC_TRY(copy_d2h(ctx, n_links_out, d + off_nl, sizeof(int) * nt));
  ISAC_TRY(copy_d2h(ctx, assoc, d + off_as, sizeof(int) * (size_t)K * nt));
  ISAC_TRY(copy_d2h(ctx, rms, d + off_rms, sizeof(double) * nt));
  if (cand_cell) ISAC_TRY(copy_d2h(ctx, cand_cell, d + off_cc, sizeof(int) * nc));
  if (cand_score) ISAC_TRY(copy_d2h(ctx, cand_score, d + off_cs, sizeof(double) * nc));
  if (cand_status) ISAC_TRY(copy_d2h(ctx, cand_status, d + off_ct, sizeof(int) * nc));
  n_out[0] = n[0];
  n_out[1] = n[1];
  return ISAC_OK;
}
