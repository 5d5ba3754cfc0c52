// Array covariance on fp64 MFMA (gfx950).
// Reference path: fft2D.m:106-111 (the eigensolvers: eigh.hip; the MUSIC scan: music.hip).
//   Ra   = X*X'/N,  X = reshape(rxGrid, N, A)'   -- the ' is a CONJUGATE transpose, so
//   Ra[a,b] = (1/N) sum_n conj(G[n,a]) G[n,b],   G[n,a] = rxGrid(n + N*a)
// Covariance: each 16x16 output tile is a real-MFMA triple on v_mfma_f64_16x16x4_f64
//   Re += Gr_I^T Gr_J + Gi_I^T Gi_J ,  Im += Gr_I^T Gi_J - Gi_I^T Gr_J
// Only tiles I <= J are formed (Hermitian).  The long sample axis n is contiguous per
// antenna column, so lane (i = lane&15, kq = lane>>4) streams 64 contiguous bytes
// (4 complex samples) of column a0+i per macro-step and feeds them to 4 consecutive MFMA
// k-steps; the k index is only a summation label, so no transposition is needed.
// Per-workgroup partial tiles are reduced in a fixed order (deterministic).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include "isac_internal.hpp"
#include "echo_dev.hpp"
#include "beam_stream.hpp"
#include "noise_walk.hpp"

namespace isac {

typedef double v4f64 __attribute__((ext_vector_type(4)));


// ---- specialised schedule for A <= 64 (NB = ceil(A/16) <= 4 antenna blocks): every wave keeps ALL blocks'
// operands of its samples in registers and owns a static group of <= 5 output tiles, so the four waves of a
// workgroup issue exactly the same number of MFMAs (balanced SIMDs), and the next slab is prefetched under the
// current slab's MFMAs.
//   wave = (tile group g, sample phase p):  NB=4: 2 groups x 2 phases,  NB=3: 2 x 2,  NB=2: 1 x 4,  NB=1: 1 x 4
//   phase p owns the contiguous samples [16 p / kPhases, 16 (p + 1) / kPhases) of a 16-sample slab -- at two phases one whole
//   128-byte line per antenna, requested by the two tile groups of that phase only; lane (i = lane&15, kq = lane>>4) holds
//   kSamplesPerLane consecutive samples of antenna 16 b + i in every block b.
// Three real MFMAs per tile and k-step instead of four (3M / Gauss form, see cov_3m_kstep): 30 instead of 40 per four samples
// at A = 64.  Measured at A = 64 (733 824 samples): 4M, interleaved sample map, 3 workgroups per CU 276 us / 1.37 GB fetched;
// 3M + line map, 2 workgroups per CU 209 us / 1.05 GB; + a workgroup barrier every 8 slabs 215 us / 0.73 GB (= the input, once).
constexpr int kCovSyncSlabs = 8;                                // power of two (1, 2, 4: +3-9 %; 16 .. none: within the noise of 8 in per-workgroup spans)
template <int NB>
struct CovPlan {
  static constexpr int kTiles = NB * (NB + 1) / 2;
  static constexpr int kGroups = (kTiles + 4) / 5;              // <= 5 tiles per wave
  static constexpr int kPerGroup = (kTiles + kGroups - 1) / kGroups;
  static constexpr int kPhases = 4 / kGroups;                   // waves per workgroup = kGroups * kPhases = 4
  static constexpr int kSamplesPerLane = 4 / kPhases;           // k-steps a wave runs per 16-sample slab
  static constexpr int first_tile(int grp) { return grp * kPerGroup; }
  static constexpr int tiles_of(int grp) { return first_tile(grp) + kPerGroup <= kTiles ? kPerGroup : kTiles - first_tile(grp); }
};

// t-th upper-triangular tile (I <= J) of an nb x nb tile grid in row-major order; the same order numbers the 64 x 64 block pairs
constexpr int cov_tile_i(int nb, int t) {
  int i = 0;
  while (t >= nb - i) { t -= nb - i; ++i; }
  return i;
}
constexpr int cov_tile_j(int nb, int t) {
  int i = 0;
  while (t >= nb - i) { t -= nb - i; ++i; }
  return i + t;
}
template <int U, int NT, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (U < NT) {
    f(std::integral_constant<int, U>{});
    static_for<U + 1, NT>(f);
  }
}

// One k-step (4 samples) of a wave's tiles T0 .. T0 + NT - 1 in 3M form: three real products per tile and k-step --
//   off-diagonal tile:  S1 += Gr_I Gr_J,  S2 += Gi_I Gi_J,  S3 += (Gr_I - Gi_I)(Gr_J + Gi_J)  =>  Re = S1 + S2,  Im = (S3 - S1) + S2
//   diagonal tile    :  Re += Gr Gr + Gi Gi,  M += Gr Gi  =>  Im = M - M^T, formed by the reducer (exactly antisymmetric)
// re = S1 (or Re), im = S2 (or M), s3 = S3 (off-diagonal tiles only; the unused ones are dead code).  The cancellation in Im is
// against terms of the size of the tile's own entries (|S1|, |S2| <~ |Re|): errors stay at a few ulp of the matrix norm.
// cur[b][E] is the operand of antenna block b, dm = Gr - Gi (row operand), sp = Gr + Gi (column operand).
// Issue order: the products of a k-step are issued tile by tile in three sweeps, so that two MFMAs into the same accumulator are
// >= 2 NT issues apart -- back-to-back dependent v_mfma_f64_16x16x4 stall for the 64-cycle pass of their predecessor.
// filler(k) is placed in the gap behind the k-th MFMA of the k-step, k = 0 .. 3 NT - 1.
template <int NB, int T0, int NT, int E, int SPL, class F>
__device__ __forceinline__ void cov_3m_kstep(const c64 (&cur)[NB][SPL], const double (&dm)[NB], const double (&sp)[NB], v4f64 (&re)[NT], v4f64 (&im)[NT],
                                             v4f64 (&s3)[NT], F&& filler) {
  static_for<0, NT>([&](auto uc) {
    constexpr int u = decltype(uc)::value;
    constexpr int I = cov_tile_i(NB, T0 + u), J = cov_tile_j(NB, T0 + u);
    re[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[I][E].re, cur[J][E].re, re[u], 0, 0, 0);
    filler(std::integral_constant<int, u>{});
  });
  static_for<0, NT>([&](auto uc) {
    constexpr int u = decltype(uc)::value;
    constexpr int I = cov_tile_i(NB, T0 + u), J = cov_tile_j(NB, T0 + u);
    if constexpr (I == J) im[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[I][E].re, cur[J][E].im, im[u], 0, 0, 0);
    else                  im[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[I][E].im, cur[J][E].im, im[u], 0, 0, 0);
    filler(std::integral_constant<int, NT + u>{});
  });
  static_for<0, NT>([&](auto uc) {
    constexpr int u = decltype(uc)::value;
    constexpr int I = cov_tile_i(NB, T0 + u), J = cov_tile_j(NB, T0 + u);
    if constexpr (I == J) re[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[I][E].im, cur[J][E].im, re[u], 0, 0, 0);
    else                  s3[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(dm[I], sp[J], s3[u], 0, 0, 0);
    filler(std::integral_constant<int, 2 * NT + u>{});
  });
}

// The two planes of a partial tile from one accumulator entry of the 3M form (see cov_3m_kstep): (Re, Im) of an off-diagonal tile, (Re, M) of a
// diagonal one -- M is antisymmetrised by the reducers.
template <bool DIAG>
__device__ __forceinline__ void cov_3m_out(double re, double im, double s3, double& o0, double& o1) {
  if constexpr (!DIAG) {
    o0 = re + im;
    o1 = (s3 - re) + im;
  } else {
    o0 = re;
    o1 = im;
  }
}

template <int NB, int GRP, int NBUF = 3>
__device__ __forceinline__ void cov_group_body(const c64* __restrict__ G, long long N, int A, int n_tiles, int phase, int lane,
                                               long long s0, long long s_step, long long s_cnt, long long s_lim, int part_index,
                                               double* __restrict__ part) {
  // this wave's i-th slab (16 samples) is slab s0 + i s_step of the grid, i = 0 .. s_cnt - 1; slabs >= s_lim contribute nothing
  using P = CovPlan<NB>;
  constexpr int T0 = P::first_tile(GRP), NT = P::tiles_of(GRP);
  constexpr int SPL = P::kSamplesPerLane;
  const int li = lane & 15, kq = lane >> 4;
  v4f64 re[NT], im[NT], s3[NT];                       // 3M accumulators (cov_3m_kstep)
#pragma unroll
  for (int u = 0; u < NT; ++u) re[u] = im[u] = s3[u] = v4f64{0.0, 0.0, 0.0, 0.0};
  // One raw-buffer descriptor per 16-antenna block (uniform: scalar registers), ending with the array's last antenna: padding antennas read as
  // zero by the bounds check, and per thread the address of all NB x SPL loads of a slab is ONE 32-bit offset (+ immediates) -- the 64-bit
  // pointer arithmetic and index clamps of a pointer-per-block form were ~30 of the ~40 VALU instructions of a slab, every one of them paid in
  // full beside the 30 v_mfma_f64 (MFMA and VALU do not co-issue).
  __amdgpu_buffer_rsrc_t rs[NB];
  bool colok[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    int n_ant = A - 16 * b;
    n_ant = n_ant < 0 ? 0 : (n_ant > 16 ? 16 : n_ant);
    colok[b] = li < n_ant;
    rs[b] = buffer_of(G + N * (long long)(n_ant > 0 ? 16 * b : 0), (unsigned)(N * n_ant * (long long)sizeof(c64)));
  }
  const long long lane_off = (16 / P::kPhases) * phase + SPL * kq;   // first sample of this lane inside a slab (see above)
  const unsigned lane_byte = (unsigned)((N * li + lane_off) * (long long)sizeof(c64));
  // Loads are unconditional (clamped indices) and the out-of-range mask is applied when a slab is CONSUMED, not when it is loaded: a
  // select at load time makes the compiler predicate the loads (branches + `s_waitcnt vmcnt(0)` before the MFMAs), a multiply at load time
  // waits for the data right away -- either way the prefetch of the next slab would not fly under the current slab's MFMAs (ISA-checked).
  // (samples past N of the last slab read the next antenna's first samples or, behind the last antenna, zero: masked at consumption)
  auto load_raw = [&](c64 (&dst)[NB][SPL], long long slab) {
    const unsigned off = lane_byte + (unsigned)slab * (unsigned)(16 * sizeof(c64));
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int e = 0; e < SPL; ++e) dst[b][e] = buffer_load_c64(rs[b], off + (unsigned)(e * sizeof(c64)));
  };
  auto mask = [&](c64 (&v)[NB][SPL], long long slab) {               // padding antennas and samples past N contribute 0
    const long long n0 = slab * 16 + lane_off;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
      for (int e = 0; e < SPL; ++e) {
        const double m = ((n0 + e < N) && colok[b] && slab < s_lim) ? 1.0 : 0.0;
        v[b][e] = mk(v[b][e].re * m, v[b][e].im * m);
      }
  };
  auto mfmas = [&](const c64 (&cur)[NB][SPL]) {
    static_for<0, SPL>([&](auto ec) {
      constexpr int e = decltype(ec)::value;
      double dm[NB], sp[NB];
#pragma unroll
      for (int b = 0; b < NB; ++b) { dm[b] = cur[b][e].re - cur[b][e].im; sp[b] = cur[b][e].re + cur[b][e].im; }
      cov_3m_kstep<NB, T0, NT, e>(cur, dm, sp, re, im, s3, [](auto) {});
    });
  };
  {
    // Three register buffers in rotation: the loads of slabs s+1 and s+2 fly under the MFMAs of slab s (one slab of MFMAs is ~0.8 us,
    // less than a loaded HBM round trip: a single prefetched slab still stalled).  Loads are unconditional (indices clamped to the
    // run's last slab): a branch around loads makes the compiler's vmcnt bookkeeping pessimistic.  Padding antennas / samples past N
    // exist only when A is not a multiple of 16 or in the very last slab: the 0/1 mask multiply runs only then (wave-uniform branch) --
    // VALU instructions do not overlap v_mfma_f64 on this hardware (tools/cobench.hip), every one of them is paid in full.
    const bool ants_full = (A == 16 * NB);
    const long long i_last = s_cnt - 1;
    auto slab_at = [&](long long i) { return s0 + (i < i_last ? i : i_last) * s_step; };
    c64 buf[NBUF][NB][SPL];                           // buffer r holds slab i with i mod NBUF == r; slabs i+1 .. i+NBUF-1 are in flight under slab i
                                                      // (NBUF = 4 fits at 254 VGPRs since the buffer loads: the same 178-182 us as NBUF = 3 at A = 64)
    auto step = [&](auto rc, long long i) {
      constexpr int r = decltype(rc)::value, f = (r + NBUF - 1) % NBUF;
      // every kCovSyncSlabs slabs the waves of the workgroup re-align, so that a line is still in L1 / L2 when the other tile group asks for
      // it (a barrier on EVERY slab costs 9-11 % of the pipelined rate: one delayed wave then stalls the workgroup each time)
      if ((i & (kCovSyncSlabs - 1)) == 0) __builtin_amdgcn_s_barrier();   // (workgroup-uniform: every wave runs s_cnt steps)
      load_raw(buf[f], slab_at(i + NBUF - 1));
      __builtin_amdgcn_sched_barrier(0);
      const long long slab = s0 + i * s_step;
      if (!ants_full || slab * 16 + 16 > N || slab >= s_lim) mask(buf[r], slab);          // (wave-uniform, rare)
      mfmas(buf[r]);
      __builtin_amdgcn_sched_barrier(0);              // waits for later slabs' data belong AFTER this slab's MFMAs have been issued
    };
    if (s_cnt > 0) static_for<0, NBUF - 1>([&](auto rc) { load_raw(buf[decltype(rc)::value], slab_at(decltype(rc)::value)); });
    long long i = 0;
    for (; i + NBUF <= s_cnt; i += NBUF) static_for<0, NBUF>([&](auto rc) { step(rc, i + decltype(rc)::value); });
    static_for<0, NBUF - 1>([&](auto rc) {
      if (i + decltype(rc)::value < s_cnt) step(rc, i + decltype(rc)::value);
    });
  }
  static_for<0, NT>([&](auto uc) {
    constexpr int u = decltype(uc)::value;
    constexpr bool diag = cov_tile_i(NB, T0 + u) == cov_tile_j(NB, T0 + u);
    double* o = part + (((long long)part_index * n_tiles + (T0 + u)) * 2) * 256;
#pragma unroll
    for (int r = 0; r < 4; ++r) cov_3m_out<diag>(re[u][r], im[u][r], s3[u][r], o[0 * 256 + r * 64 + lane], o[1 * 256 + r * 64 + lane]);
  });
}

template <int NB, int NBUF = 3>
__global__ __launch_bounds__(256, 2) void cov_mfma_small_kernel(const c64* __restrict__ G, long long N, int A,
                                                                long long slabs_per_wg,
                                                                double* __restrict__ part /* [gridX*kPhases][kTiles][2][256] */) {
  using P = CovPlan<NB>;
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int grp = wid / P::kPhases, phase = wid % P::kPhases;
  const long long total = (N + 15) / 16;
  const long long s_begin = (long long)blockIdx.x * slabs_per_wg;
  long long s_end = s_begin + slabs_per_wg;
  if (s_end > total) s_end = total;
  const int pidx = blockIdx.x * P::kPhases + phase;
  if (grp == 0) cov_group_body<NB, 0, NBUF>(G, N, A, P::kTiles, phase, lane, s_begin, 1, s_end - s_begin, s_end, pidx, part);
  if constexpr (P::kGroups > 1) {
    if (grp == 1) cov_group_body<NB, 1, NBUF>(G, N, A, P::kTiles, phase, lane, s_begin, 1, s_end - s_begin, s_end, pidx, part);
  }
}

// ---- arrays wider than 64 elements (config 4: 256-element ULA): Ra is cut into 64 x 64 blocks and every workgroup owns
// one block pair (BI <= BJ) over a chunk of samples -- a classical LDS-staged GEMM step:
//   * the 16-sample x (64 + 64)-antenna slab is fetched once per workgroup with line-friendly loads (16 consecutive lanes
//     read the 256 contiguous bytes of one antenna) into a double-buffered LDS image [block][sample][antenna ^ g(sample)], 16-slot rows
//     (kCovSwizzle below: the transposing writes and the MFMA operand reads are both conflict-free); the loads of slabs s+1, s+2
//     fly under the MFMAs of slab s; one barrier per slab;
//   * wave w computes up to four 16 x 16 tiles per slab from LDS operands: tile row w on off-diagonal blocks, a balanced
//     3/3/2/2 split of the 10 upper-triangular tiles on diagonal blocks.
// Workgroups of the same sample chunk are adjacent in the grid so that block pairs sharing an antenna block stream it
// together (Infinity Cache).  (The generic kernel above re-reads its operands once per tile triple: 8.8 ms at A = 256;
// a register-operand version of this kernel, 20 strided global loads per wave and slab: 6.4 ms.)
// LDS image: slot(block, sample, antenna) = (16 block + sample) 16 + (antenna ^ g(sample)),  g(s) = (s & 3) | (s & 4 ? 12 : 0).
//   * ds_write_b128 is served in groups of 8 contiguous lanes against 32 banks (8 slots): the lanes of a group hold samples 8h .. 8h+7 of
//     one antenna, and g's low three bits run through 0..7 there;
//   * ds_read_b128 is served in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ... against 64 banks (16 slots): a group mixes
//     antennas {0-3, 12-15} of sample quad kq with antennas {4-11} of quad kq + 1 (four samples on).  XOR with g keeps {0-3}, {4-7}, {8-11},
//     {12-15} as sets; the 12 applied on every second quad swaps {0-3} <-> {12-15} and {4-7} <-> {8-11} -- the two halves of a group land
//     on complementary slots.  (The 17-slot pitch of the first version served the writes but left every read group 2-way conflicted:
//     SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.37 at A = 256.)
constexpr int kCovPitch = 16;                                   // complex elements per (block, sample) row
__host__ __device__ constexpr int kCovSwizzle(int smp) { return (smp & 3) | ((smp & 4) ? 12 : 0); }
constexpr int kCovBufElems = 8 * 16 * kCovPitch;                // one slab image: 8 antenna blocks x 16 samples
constexpr unsigned kCovOobOffset = 0x80000000u;                 // beyond every staging descriptor (N * 256 B < 2^31, checked by the launcher)
__constant__ unsigned char kCovDiagTiles[4][4] = {              // 16*I + J per (wave, slot); 255 = idle.  Slot 0 = the wave's diagonal tile
    {0x00, 0x01, 0x02, 255}, {0x11, 0x03, 0x12, 255}, {0x22, 0x13, 255, 255}, {0x33, 0x23, 255, 255}};

// pair-th block pair (BI <= BJ) of n_blk antenna blocks, in the row-major order of cov_tile_i / cov_tile_j
__device__ __forceinline__ void cov_pair_blocks(int n_blk, int pair, int& BI, int& BJ) {
  int i = 0, rem = pair;
  while (rem >= n_blk - i) { rem -= n_blk - i; ++i; }
  BI = i;
  BJ = i + rem;
}

// Partial of tile (I, J) of a block pair -> part[chunk][pair][4 I + J][2][256].  td: the wave's diagonal tile of a diagonal pair, accumulated as
// re = Gr Gr', im = M = Gr Gi', s3 = Gi Gi' (M is antisymmetrised by cov_block_reduce_kernel); every other tile is an off-diagonal tile of the 3M form.
__device__ __forceinline__ void cov_block_tile_store(bool td, const v4f64& re, const v4f64& im, const v4f64& s3, double* __restrict__ part, int chunk,
                                                     int n_pairs, int pair, int I, int J, int lane) {
  double* o = part + ((((long long)chunk * n_pairs + pair) * 16 + (I * 4 + J)) * 2) * 256;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (td) {
      o[r * 64 + lane] = re[r] + s3[r];
      o[256 + r * 64 + lane] = im[r];
    } else {
      cov_3m_out<false>(re[r], im[r], s3[r], o[r * 64 + lane], o[256 + r * 64 + lane]);
    }
  }
}

// One block pair.  DIAG (BI == BJ) is a template parameter so that the staging loop has a compile-time trip count: with a run-time
// `j < n_stage` around the loads the wait-count pass gave up at every join and each stash waited with vmcnt(0) -- for the slab it needs AND
// for the one issued a trip later, i.e. the second slab in flight never was.  Off-diagonal pairs also lose the operand selects of the
// diagonal-tile form (VALU instructions are paid in full beside v_mfma_f64).
template <bool DIAG>
__device__ __forceinline__ void cov_block_pair(const c64* __restrict__ G, long long N, int A, int BI, int BJ, int pair, int chunk, int n_pairs,
                                               long long slabs_per_wg, double* __restrict__ part, c64* __restrict__ lds) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, kq = lane >> 4;
  // tiles of this wave: (I, J) inside the 64 x 64 block
  int tI[4], tJ[4];
  bool tv[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int code = DIAG ? (int)kCovDiagTiles[wid][u] : (16 * wid + u);
    tv[u] = !DIAG || code != 255;
    tI[u] = tv[u] ? (code >> 4) : 0;
    tJ[u] = tv[u] ? (code & 15) : 0;
  }
  constexpr int jbase = DIAG ? 0 : 4;               // LDS blocks 0..3 = antenna block BI, 4..7 = BJ (absent on diagonal pairs)
  // staging ownership: flat = j*256 + tid -> antenna slot flat/16 (0..127), sample flat%16
  constexpr int NS = DIAG ? 4 : 8;                  // loads per thread and slab
  const int s_smp = tid & 15, l16 = tid >> 4;
  // Staging step j reads antennas 64 B + 16 (j & 3) + (0..15) of block B = (j < 4 ? BI : BJ): one raw-buffer descriptor per step (uniform:
  // scalar registers) that ends with the array's last antenna, so that padding antennas read as zero by the bounds check -- per thread
  // the address is ONE 32-bit offset (N l16 + n) for all NS loads, the LDS address one base + immediate offsets.
  __amdgpu_buffer_rsrc_t s_rs[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int ant0 = 64 * (j < 4 ? BI : BJ) + 16 * (j & 3);
    int n_ant = A - ant0;
    n_ant = n_ant < 0 ? 0 : (n_ant > 16 ? 16 : n_ant);
    s_rs[j] = buffer_of(G + N * (long long)(ant0 < A ? ant0 : 0), (unsigned)(N * n_ant * (long long)sizeof(c64)));
  }
  const int s_lds0 = s_smp * kCovPitch + (l16 ^ kCovSwizzle(s_smp));       // + j * 16 * kCovPitch
  // 3M form, as in cov_3m_kstep: off-diagonal tile re = S1, im = S2, s3 = S3; diagonal tile (slot 0 of every wave of a diagonal block
  // pair: a compile-time property, so neither selects nor branch-dependent accumulator moves) re + s3 = Re, im = M.
  v4f64 re[4], im[4], s3[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) re[u] = im[u] = s3[u] = v4f64{0.0, 0.0, 0.0, 0.0};
  const long long total = (N + 15) / 16;
  const long long s_begin = (long long)chunk * slabs_per_wg;
  long long s_end = s_begin + slabs_per_wg;
  if (s_end > total) s_end = total;
  // Two slabs of global loads in flight (register sets gA / gB in rotation): one slab of MFMAs is ~1.3 us, less than a loaded HBM round
  // trip -- with a single prefetched slab (round 2) the stash of slab s + 1 still waited for its loads (0.52 of the MFMA peak at A = 256).
  // Samples past N and whole slabs past the chunk's end are fetched at an offset beyond every descriptor: they read as zero without a
  // select behind the load (a select is a use of the loaded value and puts the wait for it right there) and without memory traffic.
  c64 gA[NS], gB[NS];
  auto fetch = [&](c64 (&g)[NS], long long slab) {
    const long long n = slab * 16 + s_smp;
    const unsigned voff = (n < N && slab < s_end) ? (unsigned)((N * l16 + n) * (long long)sizeof(c64)) : kCovOobOffset;
#pragma unroll
    for (int j = 0; j < NS; ++j) g[j] = buffer_load_c64(s_rs[j], voff);
  };
  auto stash = [&](const c64 (&g)[NS], int buf) {
    c64* d = lds + buf * kCovBufElems + s_lds0;
#pragma unroll
    for (int j = 0; j < NS; ++j) d[j * 16 * kCovPitch] = g[j];
  };
  int r_off[4];                                     // operand slot of this lane for sample 4 kq + e inside a (block, 16-sample) image
#pragma unroll
  for (int e = 0; e < 4; ++e) r_off[e] = (4 * kq + e) * kCovPitch + (li ^ kCovSwizzle(4 * kq + e));
  auto mfmas = [&](int buf) {
    const c64* cur = lds + buf * kCovBufElems;
    if constexpr (!DIAG) {
      // off-diagonal pair: wave w owns tile row w (tI = w, tJ = 0..3) -- the row operand is read once per sample quad and shared by
      // the four tiles: 20 instead of 32 ds_read_b128 per slab, and the operand registers of one quad at a time
      const c64* pa = cur + wid * 16 * kCovPitch;
      const c64* pb = cur + jbase * 16 * kCovPitch;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const c64 xa = pa[r_off[e]];
        const double dm = xa.re - xa.im;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const c64 xb = pb[u * 16 * kCovPitch + r_off[e]];
          re[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa.re, xb.re, re[u], 0, 0, 0);
          im[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa.im, xb.im, im[u], 0, 0, 0);
          s3[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(dm, xb.re + xb.im, s3[u], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);          // operand reads of at most one quad ahead of their MFMAs (register budget)
      }
    } else {
      {                                             // slot 0: the wave's diagonal tile -- Gr Gr', M = Gr Gi', Gi Gi'
        const c64* pa = cur + tI[0] * 16 * kCovPitch;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const c64 xa = pa[r_off[e]];
          re[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa.re, xa.re, re[0], 0, 0, 0);
          im[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa.re, xa.im, im[0], 0, 0, 0);
          s3[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa.im, xa.im, s3[0], 0, 0, 0);
        }
      }
#pragma unroll
      for (int u = 1; u < 3; ++u) {                 // slots 1, 2: off-diagonal tiles (slot 2 on waves 0 and 1 only; slot 3 is never used)
        if (u == 2 && !tv[2]) continue;             // (wave-uniform)
        const c64* pa = cur + tI[u] * 16 * kCovPitch;
        const c64* pb = cur + tJ[u] * 16 * kCovPitch;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const c64 xa = pa[r_off[e]], xb = pb[r_off[e]];
          re[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa.re, xb.re, re[u], 0, 0, 0);
          im[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa.im, xb.im, im[u], 0, 0, 0);
          s3[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa.re - xa.im, xb.re + xb.im, s3[u], 0, 0, 0);
        }
      }
    }
  };
  // Two trips per iteration, no exit in the middle (an odd slab count runs one all-zero slab): the accumulators keep their registers
  // over the back-edge -- with a mid-loop exit the compiler moved all twelve of them, 48 v_mov_b64 per trip, paid in full beside the MFMAs.
  if (s_begin < s_end) {
    fetch(gA, s_begin);
    stash(gA, 0);
    fetch(gA, s_begin + 1);
    fetch(gB, s_begin + 2);
  }
  __syncthreads();
  for (long long slab = s_begin; slab < s_end; slab += 2) {
    // even trip: slab from buffer 0; gA holds slab + 1 (issued two trips ago), gB slab + 2 (in flight)
    mfmas(0);
    stash(gA, 1);
    fetch(gA, slab + 3);
    __syncthreads();
    // odd trip: slab + 1 from buffer 1; gB holds slab + 2
    mfmas(1);
    stash(gB, 0);
    fetch(gB, slab + 4);
    __syncthreads();
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    if (DIAG && !tv[u]) continue;
    cov_block_tile_store(DIAG && u == 0, re[u], im[u], s3[u], part, chunk, n_pairs, pair, tI[u], tJ[u], lane);
  }
}

// ---- the same block pairs, software-pipelined inside the wave (round 4; the shipped kernel for A > 64, cov_block_pair above stays as the
// fallback for sample counts beyond this kernel's 32-bit staging offsets).  cov_block_pair issues, per 16-sample slab and wave,
// [5 ds_read, wait, 12 MFMAs] x 4, then 8 ds_write + 8 loads + barrier: on gfx950 a wave that wants to issue a v_mfma_f64 into the busy pipe
// holds the SIMD's issue port, so nothing of the OTHER workgroup's wave hides those bursts (tools/cobench.hip: together = sum for LDS and
// global-memory instructions too) -- 0.53 of the MFMA peak at A = 256.  Here the pipeline step is ONE k-step (4 samples: 12 MFMAs on an
// off-diagonal pair) on operands read during the step before, and its gaps carry, one instruction each, the operand reads of the next k-step,
// a quarter of the staging writes of the unit after next and the re-issue of those staging loads.  Unit = 8 samples (two k-steps); four
// 16 KB images in rotation (the same 64 KB): unit u is read during u - 1 / u, unit u + 2 written during u, one barrier per unit.
// Image of a unit: [antenna block 0..7][sample 0..7][antenna ^ g(sample)] (16-slot rows, kCovSwizzle): staging writes (8 lanes = the 8
// samples of one antenna) and operand reads (sample 4 e + kq) are conflict-free as in the 16-sample image.
constexpr int kCovUnit = 8;
constexpr int kCovUBlk = kCovUnit * kCovPitch;                  // complex elements per (antenna block, unit)
constexpr int kCovUImg = 8 * kCovUBlk;                          // one image (16 KB)
constexpr int kCovUImgs = 4;
template <bool DIAG, int NSLOT>                                 // NSLOT: tiles of this wave -- 4 on an off-diagonal pair, 3 / 2 on a diagonal one (waves 0, 1 / 2, 3)
__device__ __forceinline__ void cov_block_pair_pl(const c64* __restrict__ G, long long N, int A, int BI, int BJ, int pair, int chunk, int n_pairs,
                                                  long long units_per_wg, double* __restrict__ part, c64* __restrict__ lds) {
  static_assert(DIAG ? (NSLOT == 2 || NSLOT == 3) : NSLOT == 4, "");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, kq = lane >> 4;
  int tI[NSLOT], tJ[NSLOT];
#pragma unroll
  for (int u = 0; u < NSLOT; ++u) {
    const int code = DIAG ? (int)kCovDiagTiles[wid][u] : (16 * wid + u);
    tI[u] = code >> 4;
    tJ[u] = code & 15;
  }
  // operands of one k-step.  Off-diagonal pair: op 0 = the wave's row tile (LDS block wid), op 1 + u = column tile u (LDS block 4 + u).
  // Diagonal pair: op 0 = the diagonal tile (slot 0), ops 2 u - 1, 2 u = row / column tile of slot u >= 1.
  constexpr int NOP = DIAG ? 2 * NSLOT - 1 : 1 + NSLOT;
  int a_off[NOP][2];                                // element offset of operand i, k-step e inside an image
#pragma unroll
  for (int i = 0; i < NOP; ++i) {
    int blk;
    if constexpr (DIAG) blk = i == 0 ? tI[0] : ((i & 1) ? tI[(i + 1) >> 1] : tJ[i >> 1]);
    else blk = i == 0 ? wid : 3 + i;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int smp = 4 * e + kq;
      a_off[i][e] = blk * kCovUBlk + smp * kCovPitch + (li ^ kCovSwizzle(smp));
    }
  }
  // staging: load j of a unit covers antennas 32 j .. 32 j + 31 of the pair's 128 (64) x the unit's 8 samples -- thread -> (sample tid & 7,
  // antenna tid >> 3); 8 consecutive lanes read one 128-byte line.  One descriptor per load (uniform), ending with the array's last antenna.
  constexpr int NS = DIAG ? 2 : 4;
  const int s_smp = tid & 7, l32 = tid >> 3;
  __amdgpu_buffer_rsrc_t s_rs[NS];
#pragma unroll
  for (int j = 0; j < NS; ++j) {
    const int ant0 = 64 * (j < 2 ? BI : BJ) + 32 * (j & 1);
    int n_ant = A - ant0;
    n_ant = n_ant < 0 ? 0 : (n_ant > 32 ? 32 : n_ant);
    s_rs[j] = buffer_of(G + N * (long long)(ant0 < A ? ant0 : 0), (unsigned)(N * n_ant * (long long)sizeof(c64)));
  }
  const int s_lds0 = ((l32 >> 4) * kCovUnit + s_smp) * kCovPitch + ((l32 & 15) ^ kCovSwizzle(s_smp));   // + 2 j kCovUBlk: LDS block 2 j + (l32 >> 4)
  const long long total = (N + kCovUnit - 1) / kCovUnit;
  const long long u_begin = (long long)chunk * units_per_wg;
  long long u_end = u_begin + units_per_wg;
  if (u_end > total) u_end = total;
  auto voff_of = [&](long long unit) {               // samples past N / units past the chunk: an offset beyond every descriptor reads zero
    const long long n = unit * kCovUnit + s_smp;
    return (n < N && unit < u_end) ? (unsigned)((N * l32 + n) * (long long)sizeof(c64)) : kCovOobOffset;
  };
  v4f64 re[NSLOT], im[NSLOT], s3[NSLOT];             // 3M form as in cov_block_pair: off-diagonal tile S1, S2, S3; diagonal tile (slot 0) Gr Gr', M, Gi Gi'
#pragma unroll
  for (int u = 0; u < NSLOT; ++u) re[u] = im[u] = s3[u] = v4f64{0.0, 0.0, 0.0, 0.0};
  c64 g[2][NS];                                      // staging sets: during unit u, g[u & 1] holds unit u + 2 (then u + 4), the other u + 3
  c64 ops[2][NOP];                                   // operand sets by k-step parity
  // One k-step.  UQ = unit index mod 4 (its image), E = k-step of the unit: compile time, the loop below is unrolled over four units.
  auto kstep = [&](auto uq_c, auto e_c, long long unit) {
    constexpr int UQ = decltype(uq_c)::value, E = decltype(e_c)::value, SET = UQ & 1;
    constexpr int IMG_RD = E == 0 ? UQ : ((UQ + 1) & 3), E_RD = E ^ 1, IMG_WR = (UQ + 2) & 3;
    const c64 (&cur)[NOP] = ops[E];
    c64 (&nxt)[NOP] = ops[E ^ 1];
    const unsigned voff = voff_of(unit + 4);
    double dm[NSLOT], sp[NSLOT];                     // Gr - Gi of the row operand, Gr + Gi of the column operand (slot 0 of a diagonal pair: unused)
#pragma unroll
    for (int u = DIAG ? 1 : 0; u < NSLOT; ++u) {
      const c64 xa = DIAG ? cur[2 * u - 1] : cur[0], xb = DIAG ? cur[2 * u] : cur[1 + u];
      dm[u] = xa.re - xa.im;
      sp[u] = xb.re + xb.im;
    }
    __builtin_amdgcn_sched_barrier(0);
    // filler k sits in the gap behind the k-th MFMA of the k-step: the NOP operand reads of the next k-step, NS / 2 staging writes, NS / 2 staging loads
    auto filler = [&](auto kc) {
      constexpr int k = decltype(kc)::value;
      if constexpr (k < NOP) {
        nxt[k] = lds[IMG_RD * kCovUImg + a_off[k][E_RD]];
        __builtin_amdgcn_sched_barrier(0);
      } else if constexpr (k < NOP + NS / 2) {
        constexpr int j = E * (NS / 2) + (k - NOP);
        lds[IMG_WR * kCovUImg + s_lds0 + 2 * j * kCovUBlk] = g[SET][j];
        __builtin_amdgcn_sched_barrier(0);
      } else if constexpr (k < NOP + NS) {
        constexpr int j = E * (NS / 2) + (k - NOP - NS / 2);
        g[SET][j] = buffer_load_c64(s_rs[j], voff);
        __builtin_amdgcn_sched_barrier(0);
      }
    };
    static_assert(3 * NSLOT >= NOP + NS, "every filler has its gap");
    static_for<0, NSLOT>([&](auto uc) {
      constexpr int u = decltype(uc)::value;
      if constexpr (DIAG && u == 0) re[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[0].re, cur[0].re, re[0], 0, 0, 0);
      else if constexpr (DIAG) re[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[2 * u - 1].re, cur[2 * u].re, re[u], 0, 0, 0);
      else re[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[0].re, cur[1 + u].re, re[u], 0, 0, 0);
      filler(std::integral_constant<int, u>{});
    });
    static_for<0, NSLOT>([&](auto uc) {
      constexpr int u = decltype(uc)::value;
      if constexpr (DIAG && u == 0) im[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[0].re, cur[0].im, im[0], 0, 0, 0);
      else if constexpr (DIAG) im[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[2 * u - 1].im, cur[2 * u].im, im[u], 0, 0, 0);
      else im[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[0].im, cur[1 + u].im, im[u], 0, 0, 0);
      filler(std::integral_constant<int, NSLOT + u>{});
    });
    static_for<0, NSLOT>([&](auto uc) {
      constexpr int u = decltype(uc)::value;
      if constexpr (DIAG && u == 0) s3[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[0].im, cur[0].im, s3[0], 0, 0, 0);
      else s3[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(dm[u], sp[u], s3[u], 0, 0, 0);
      filler(std::integral_constant<int, 2 * NSLOT + u>{});
    });
    if constexpr (E == 1) __syncthreads();
  };
  auto fetch = [&](c64 (&gg)[NS], long long unit) {
    const unsigned voff = voff_of(unit);
#pragma unroll
    for (int j = 0; j < NS; ++j) gg[j] = buffer_load_c64(s_rs[j], voff);
  };
  auto stash = [&](const c64 (&gg)[NS], int img) {
#pragma unroll
    for (int j = 0; j < NS; ++j) lds[img * kCovUImg + s_lds0 + 2 * j * kCovUBlk] = gg[j];
  };
  // prologue: units 0, 1 -> images 0, 1; units 2, 3 in flight; operands of (unit 0, k-step 0)
  fetch(g[0], u_begin);
  fetch(g[1], u_begin + 1);
  stash(g[0], 0);
  stash(g[1], 1);
  fetch(g[0], u_begin + 2);
  fetch(g[1], u_begin + 3);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < NOP; ++i) ops[0][i] = lds[a_off[i][0]];
  for (long long unit = u_begin; unit < u_end; unit += 4) {     // (a unit count that is no multiple of four runs all-zero units: no exit in the middle)
    static_for<0, 4>([&](auto uq_c) {
      kstep(uq_c, std::integral_constant<int, 0>{}, unit + decltype(uq_c)::value);
      kstep(uq_c, std::integral_constant<int, 1>{}, unit + decltype(uq_c)::value);
    });
  }
#pragma unroll
  for (int u = 0; u < NSLOT; ++u) cov_block_tile_store(DIAG && u == 0, re[u], im[u], s3[u], part, chunk, n_pairs, pair, tI[u], tJ[u], lane);
}

__global__ __launch_bounds__(256, 2) void cov_mfma_block_pl_kernel(const c64* __restrict__ G, long long N, int A, int n_blk, int n_pairs,
                                                                   long long units_per_wg, double* __restrict__ part /* [chunk][pair][16][2][256] */) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  c64* lds = reinterpret_cast<c64*>(smem_raw);      // [kCovUImgs][kCovUImg]
  const int pair = blockIdx.x % n_pairs, chunk = blockIdx.x / n_pairs;
  int BI, BJ;
  cov_pair_blocks(n_blk, pair, BI, BJ);
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (BI != BJ) cov_block_pair_pl<false, 4>(G, N, A, BI, BJ, pair, chunk, n_pairs, units_per_wg, part, lds);
  else if (wid < 2) cov_block_pair_pl<true, 3>(G, N, A, BI, BJ, pair, chunk, n_pairs, units_per_wg, part, lds);
  else cov_block_pair_pl<true, 2>(G, N, A, BI, BJ, pair, chunk, n_pairs, units_per_wg, part, lds);
}

// ---- 33..64 antennas (NB = 3, 4: two tile groups), LDS-staged and software-pipelined INSIDE the wave (round 4).
// Two measurements of this round decide the shape (profiles/r04_cobench.txt, r04_gbench.txt, r04_cov_probe_variants.txt):
//  * cov_mfma_small_kernel feeds the MFMAs from registers: lane (i, kq) loads its own operand, i.e. 16 consecutive lanes read 16 different
//    antenna columns, 16 bytes each.  The texture path serves such a gather at about one lane per cycle (64 cycles per wave instruction where a
//    coalesced 1 KB load takes 16), and with two tile groups both waves of a sample phase load (nearly) every block: the loads alone take
//    152-173 us of that kernel's 190.  Here a slab (16 samples x 64 antennas = 16 KB) is fetched ONCE per workgroup with coalesced loads
//    (16 lanes read 256 contiguous bytes of one antenna, 4 loads per thread), transposed through the block kernel's swizzled LDS image, and
//    every wave reads its operands with ds_read_b128 (conflict-free, 6-8 per slab).
//  * A wave that wants to issue a v_mfma_f64 into the busy pipe holds the SIMD's issue port: beside a wave that streams MFMAs, ANOTHER wave's
//    ds_read / ds_write / global loads cost their full stand-alone time (cobench: together = sum for every instruction kind, not only VALU).  A
//    kernel whose waves alternate "burst of memory instructions" / "run of 30 MFMAs" therefore leaves the pipe idle while both waves of a SIMD do
//    their bursts one after the other -- the first staged version of this kernel (burst form) ran 193 us; without its barriers 180, without its
//    staging instructions 170, as a bare MFMA stream 159.  The fix is to hide every non-MFMA instruction in the 64-cycle shadow of the wave's OWN
//    MFMAs: each slab step issues its 30 MFMAs on operands already in registers and, one instruction per MFMA gap, reads the NEXT slab's operands
//    from LDS, writes the slab after that into LDS and re-issues the global loads (sched_barrier pins the positions).
// Three LDS images in rotation (operands of slab s + 1 are read while slab s + 2 is written: one barrier per slab covers both hazards), two
// staging register sets (two slabs of global loads in flight), two operand register sets.  Same tile groups / sample phases / 3M accumulators /
// partial layout as cov_group_body, so the reducers are shared; a phase owns the k-steps e = 2 p, 2 p + 1 of the image (samples {e, 4 + e, 8 + e, 12 + e}).
constexpr int kCovLdsBufs = 3;
constexpr int kCovSlabBlk = 16 * kCovPitch;                     // one 16-antenna block of a slab image (an image: NB of them)

// The phase exchange and partial store of a staged tile group: the two sample phases of a tile group are summed inside the workgroup (through the now idle
// slab images) before anything goes to memory: one partial per workgroup and tile instead of two -- half the partial-sum traffic of the kernel and of the
// reducers behind it (20 instead of 41 MB per launch at A = 64).
template <int NB, int GRP, int NT>
__device__ __forceinline__ void cov_phase_sum_store(const v4f64 (&re)[NT], const v4f64 (&im)[NT], const v4f64 (&s3)[NT], int phase, int lane, int part_index,
                                                    double* __restrict__ part, c64* __restrict__ lds) {
  using P = CovPlan<NB>;
  constexpr int T0 = P::first_tile(GRP);
  double* x = reinterpret_cast<double*>(lds) + GRP * (P::kPerGroup * 2 * 256);
  static_assert(sizeof(c64) * kCovLdsBufs * NB * kCovSlabBlk >= sizeof(double) * 2 * P::kPerGroup * 2 * 256, "the phase exchange fits the slab images");
  double o0[NT][4], o1[NT][4];
  static_for<0, NT>([&](auto uc) {
    constexpr int u = decltype(uc)::value;
    constexpr bool diag = cov_tile_i(NB, T0 + u) == cov_tile_j(NB, T0 + u);
#pragma unroll
    for (int r = 0; r < 4; ++r) cov_3m_out<diag>(re[u][r], im[u][r], s3[u][r], o0[u][r], o1[u][r]);
  });
  if (phase == 1) {
#pragma unroll
    for (int u = 0; u < NT; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) { x[(u * 2 + 0) * 256 + r * 64 + lane] = o0[u][r]; x[(u * 2 + 1) * 256 + r * 64 + lane] = o1[u][r]; }
  }
  __syncthreads();
  if (phase == 0) {
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      double* o = part + (((long long)part_index * P::kTiles + (T0 + u)) * 2) * 256;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        o[0 * 256 + r * 64 + lane] = o0[u][r] + x[(u * 2 + 0) * 256 + r * 64 + lane];
        o[1 * 256 + r * 64 + lane] = o1[u][r] + x[(u * 2 + 1) * 256 + r * 64 + lane];
      }
    }
  }
}

// One wave of a staged kernel: tile group GRP, sample phase `phase`, slabs s_begin .. s_end - 1 of the workgroup.  Each slab step issues its 6 NT MFMAs (30 at
// NB = 4) on operands already in registers; filler k goes into the gap behind the k-th MFMA of the step: gaps 0 .. 2 NB - 1 the operand reads of the next slab,
// the gaps behind them whatever the Source needs to put the slab after that into its LDS image (sched_barrier pins the positions of the first Source::kGaps).
// A Source provides
//   prologue(lds)                   slabs s_begin, s_begin + 1 -> images 0, 1; slabs s_begin + 2, s_begin + 3 in flight
//   begin_step(slab)                in front of the MFMAs of `slab`
//   gap<PAR, K>(dst_image, slab)    its share of gap K of the step for `slab` (PAR = the step's parity: register sets), building slab + 2 in dst_image
template <int NB, int GRP, class Source>
__device__ __forceinline__ void cov_staged_body(Source src, int phase, long long s_begin, long long s_end, int part_index, double* __restrict__ part,
                                                c64* __restrict__ lds) {
  using P = CovPlan<NB>;
  static_assert(P::kGroups == 2 && P::kPhases == 2, "two tile groups x two sample phases");
  constexpr int T0 = P::first_tile(GRP), NT = P::tiles_of(GRP);
  constexpr int kBuf = NB * kCovSlabBlk;            // one slab image
  static_assert(6 * NT >= Source::kGaps && Source::kGaps >= 2 * NB, "every filler has its gap");
  const int lane = threadIdx.x & 63;
  const int li = lane & 15, kq = lane >> 4;
  v4f64 re[NT], im[NT], s3[NT];
#pragma unroll
  for (int u = 0; u < NT; ++u) re[u] = im[u] = s3[u] = v4f64{0.0, 0.0, 0.0, 0.0};
  int r_off[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int smp = 4 * kq + 2 * phase + e;
    r_off[e] = smp * kCovPitch + (li ^ kCovSwizzle(smp));
  }
  c64 ops[2][NB][2];                                 // operand sets: ops[s & 1] holds slab s
  // One slab step.  PAR = parity of the step (compile time: register sets), rd / wr = LDS images of slab + 1 (complete) and slab + 2 (free).
  auto step = [&](auto par_c, long long slab, int rd, int wr) {
    constexpr int PAR = decltype(par_c)::value;
    const c64 (&cur)[NB][2] = ops[PAR];
    c64 (&nxt)[NB][2] = ops[PAR ^ 1];
    const c64* img = lds + rd * kBuf;
    c64* dst = lds + wr * kBuf;
    src.begin_step(slab);
    double dm[2][NB], sp[2][NB];                     // Gr - Gi (row operand), Gr + Gi (column operand) of the 3M form
#pragma unroll
    for (int e = 0; e < 2; ++e)
#pragma unroll
      for (int b = 0; b < NB; ++b) { dm[e][b] = cur[b][e].re - cur[b][e].im; sp[e][b] = cur[b][e].re + cur[b][e].im; }
    __builtin_amdgcn_sched_barrier(0);
    static_for<0, 2>([&](auto ec) {
      constexpr int e = decltype(ec)::value;
      cov_3m_kstep<NB, T0, NT, e>(cur, dm[e], sp[e], re, im, s3, [&](auto kc) {
        constexpr int k = e * 3 * NT + decltype(kc)::value;
        if constexpr (k < 2 * NB) nxt[k % NB][k / NB] = img[(k % NB) * kCovSlabBlk + r_off[k / NB]];   // (blocks no tile of this group touches: dead reads, dropped by the compiler)
        src.template gap<PAR, k>(dst, slab);
        if constexpr (k < Source::kGaps) __builtin_amdgcn_sched_barrier(0);
      });
    });
    __syncthreads();
  };
  src.prologue(lds);
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 2; ++e)
#pragma unroll
    for (int b = 0; b < NB; ++b) ops[0][b][e] = lds[b * kCovSlabBlk + r_off[e]];
  int rd = 1, wr = 2;                                // (uniform) image of slab + 1, image for slab + 2
  auto rot = [&]() { rd = wr; wr = wr == kCovLdsBufs - 1 ? 0 : wr + 1; };
  for (long long slab = s_begin; slab < s_end; slab += 2) {       // (an odd slab count runs one all-zero slab: no exit in the middle)
    step(std::integral_constant<int, 0>{}, slab, rd, wr);
    rot();
    step(std::integral_constant<int, 1>{}, slab + 1, rd, wr);
    rot();
  }
  cov_phase_sum_store<NB, GRP>(re, im, s3, phase, lane, part_index, part, lds);
}

// The slab source of cov_mfma_lds_kernel: the grid in memory.  thread -> (sample tid & 15, antenna 16 j + (tid >> 4)), j = 0 .. NB - 1; one descriptor per
// 16-antenna block that ends with the array's last antenna (padding antennas read as zero by the bounds check).  Gaps 2 NB .. 3 NB - 1 carry the NB staging
// writes, gaps 3 NB .. 4 NB - 1 the NB staging loads into the registers just written out.
template <int NB>
struct CovArrayStager {
  static constexpr int kGaps = 4 * NB;
  __amdgpu_buffer_rsrc_t s_rs[NB];
  c64 g[2][NB];                                      // staging sets: at the top of the step for slab s, g[s & 1] holds slab s + 2, the other s + 3
  long long N, row, s_begin, s_end;                  // row = N (tid >> 4): first sample of this thread's antenna inside a block
  int s_smp, s_lds0;
  unsigned voff;                                     // of the loads of the running step
  __device__ __forceinline__ CovArrayStager(const c64* __restrict__ G, long long N_, int A, long long s_begin_, long long s_end_)
      : N(N_), row(N_ * (threadIdx.x >> 4)), s_begin(s_begin_), s_end(s_end_), s_smp(threadIdx.x & 15) {
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      int n_ant = A - 16 * j;
      n_ant = n_ant < 0 ? 0 : (n_ant > 16 ? 16 : n_ant);
      s_rs[j] = buffer_of(G + N * (long long)(n_ant > 0 ? 16 * j : 0), (unsigned)(N * n_ant * (long long)sizeof(c64)));
    }
    s_lds0 = s_smp * kCovPitch + ((threadIdx.x >> 4) ^ kCovSwizzle(s_smp));
  }
  __device__ __forceinline__ unsigned voff_of(long long slab) const {   // samples past N / slabs past the chunk: an offset beyond every descriptor reads zero
    const long long n = slab * 16 + s_smp;
    return (n < N && slab < s_end) ? (unsigned)((row + n) * (long long)sizeof(c64)) : kCovOobOffset;
  }
  __device__ __forceinline__ void fetch(c64 (&gg)[NB], long long slab) {
    const unsigned v = voff_of(slab);
#pragma unroll
    for (int j = 0; j < NB; ++j) gg[j] = buffer_load_c64(s_rs[j], v);
  }
  __device__ __forceinline__ void stash(const c64 (&gg)[NB], c64* img) {
    c64* d = img + s_lds0;
#pragma unroll
    for (int j = 0; j < NB; ++j) d[j * kCovSlabBlk] = gg[j];
  }
  __device__ __forceinline__ void prologue(c64* __restrict__ lds) {
    // The loads of the two slabs in flight are issued slab by slab, as the steps re-issue them: interleaved, the vmcnt waits of every step cover both slabs.
    // The sched_barrier holds the order only if no load is moved behind the slab loop's guard: every workgroup of a launch has a slab, said here.
    __builtin_assume(s_begin < s_end);
    fetch(g[0], s_begin);
    fetch(g[1], s_begin + 1);
    stash(g[0], lds);
    stash(g[1], lds + NB * kCovSlabBlk);
    fetch(g[0], s_begin + 2);
    __builtin_amdgcn_sched_barrier(0);
    fetch(g[1], s_begin + 3);
  }
  __device__ __forceinline__ void begin_step(long long slab) { voff = voff_of(slab + 4); }
  template <int PAR, int K>
  __device__ __forceinline__ void gap(c64* dst, long long) {
    if constexpr (K >= 2 * NB && K < 3 * NB) dst[s_lds0 + (K - 2 * NB) * kCovSlabBlk] = g[PAR][K - 2 * NB];
    else if constexpr (K >= 3 * NB && K < 4 * NB) g[PAR][K - 3 * NB] = buffer_load_c64(s_rs[K - 3 * NB], voff);
  }
};

template <int NB>
__global__ __launch_bounds__(256, 2) void cov_mfma_lds_kernel(const c64* __restrict__ G, long long N, int A, long long slabs_per_wg,
                                                              double* __restrict__ part /* [gridX][kTiles][2][256] */) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  c64* lds = reinterpret_cast<c64*>(smem_raw);      // [kCovLdsBufs][NB * kCovSlabBlk]
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int grp = wid >> 1, phase = wid & 1;
  const long long total = (N + 15) / 16;
  const long long s_begin = (long long)blockIdx.x * slabs_per_wg;
  long long s_end = s_begin + slabs_per_wg;
  if (s_end > total) s_end = total;
  const int pidx = blockIdx.x;                       // (one partial per workgroup: the phases are summed in the kernel)
  if (grp == 0) cov_staged_body<NB, 0>(CovArrayStager<NB>(G, N, A, s_begin, s_end), phase, s_begin, s_end, pidx, part, lds);
  else cov_staged_body<NB, 1>(CovArrayStager<NB>(G, N, A, s_begin, s_end), phase, s_begin, s_end, pidx, part, lds);
}

// ---------------------------------------------------------------- covariance of a LAZY echo grid (round 6)
// The fused monoStaticSensing call wrote echoGrid (0.75 GB at the bench shape) only so that this stage could read it back.  With the spectral noise route the grid is a function
// of 12 MB of inputs:   e[k, l, r] = sum_q D_q[k, l] a_q[r] + sig W(seed; k, l, r),   W = float32 Box-Muller of one Philox4x32-10 call per element PAIR (k, k + 512)
// (echo_dev.hpp).  cov_lazy_kernel is cov_mfma_lds_kernel<4> with the slab staging (four 16-byte global loads per thread and slab) replaced by a generator that re-forms the
// slab's 16 x 64 elements with THE expression of the synthesis kernel (spectral_echo_value: the same bits) and writes them into the same swizzled LDS image:
//   * a slab is 8 PAIR rows of one symbol column: samples k0 + p and k0 + p + 512 (p = 0..7) occupy sample slots p and p + 8, so that both halves of every Philox call are
//     used -- the slab order is therefore (symbol, 1024-subcarrier block pair, 8-row group), not the flat n = k + K l of the array form; the sum is the same, its rounding
//     differs in the last bits (tests: <= 1e-13 of the array form; every estimate identical).  K is not a multiple of 1024: the partner half of the last block pair is masked
//     (218 instead of 204.75 slabs per column at K = 3276: 6 % more MFMA issue than the array form);
//   * thread (p = tid & 7, r0 = tid >> 3) makes TWO Philox calls per slab -- antennas r0 and r0 + 32 -- i.e. four elements, and two 16-byte loads of D (from L2: the lanes of a
//     wave share 8 subcarriers) per target, issued two slabs ahead;
//   * the generator is cut into 19 pieces (counter set-up + 10 Philox rounds, 4 Box-Muller transforms, 4 x (synthesis + mask + LDS store), the D loads) that sit in the gaps of the
//     step's 30 MFMAs like the staging instructions did, spread evenly (lazy_piece_gap).
// Bound: fp64 MFMA issue + the generator's VALU (v_mfma_f64 and VALU of one wave overlap only inside the 64-cycle shadow of the wave's own MFMA, section 3d of DESIGN_HISTORY.md).
struct LazyCovArgs {
  const c64* D;               // [K x L_whole x QT] per-target demodulated coefficient grids
  const c64* steer_rq;        // [A x QT]: a_q[r] at r QT + q
  double sig;
  unsigned long long seed;
  int K, L_whole, L_out, A;
  int s_col;                  // slabs per symbol column
};
constexpr int kLazyPieces = 19;
__host__ __device__ constexpr int lazy_piece_gap(int i) {       // MFMA gap (0..29) that carries generator piece i
  return (i * 30) / kLazyPieces;
}

// The slab source of cov_lazy_kernel: thread -> (pair row gp, antennas ga and ga + 32) of every slab.
// (CovNoiseBeamSource below restates its cursor, counter, mask, Philox and Box-Muller members: the noise field of the two routes is the same only while the two stay in step --
//  tests/test_gpu_lazy_split.py compares them.  They are two texts because this struct's kernel is pinned instruction by instruction.)
template <int QT>
struct CovLazyGenerator {
  static constexpr int NB = 4;
  static constexpr int kGaps = 30;                   // the generator's pieces are spread over all 30 gaps of a step (lazy_piece_gap)
  struct Cur { int l, sc; long long g; };            // slab g = slab sc of symbol column l
  int gp, ga, K, s_col, g_lds0;
  double sig;
  uint32_t key0, key1;
  long long s_end;
  c64 st[2][QT];
  bool ant_ok[2];
  uint64_t colbase[2];
  __amdgpu_buffer_rsrc_t rsD[QT];
  Cur cg, cd;                                        // cursors (wave-uniform): the slab being generated and the slab whose D values are being fetched
  uint32_t pc[2][4];
  float wf[2][2][2];
  bool v_half[2];
  c64 dl[2][QT][2];                                  // D values of two slabs in flight: dl[par][q][half]
  __device__ __forceinline__ CovLazyGenerator(const LazyCovArgs& a, long long s_begin, long long s_end_)
      : gp(threadIdx.x & 7), ga(threadIdx.x >> 3), K(a.K), s_col(a.s_col), sig(a.sig), key0((uint32_t)a.seed), key1((uint32_t)(a.seed >> 32)), s_end(s_end_) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ant = ga + 32 * j;
      ant_ok[j] = ant < a.A;
      colbase[j] = (uint64_t)gp + (uint64_t)kSpectralSlotsPerColumn * ((uint64_t)a.L_out * (uint64_t)ant);   // the thread's part of the Philox counter; the slab's part (init) is wave-uniform
#pragma unroll
      for (int q = 0; q < QT; ++q) st[j][q] = ant_ok[j] ? a.steer_rq[(long long)ant * QT + q] : mk(0.0, 0.0);
    }
#pragma unroll
    for (int q = 0; q < QT; ++q) rsD[q] = buffer_of(a.D + (long long)q * K * a.L_whole, (unsigned)((long long)K * a.L_whole * (long long)sizeof(c64)));
    g_lds0 = (ga >> 4) * kCovSlabBlk + gp * kCovPitch + ((ga & 15) ^ kCovSwizzle(gp));     // element (antenna ga, sample slot gp); + 2 j kCovSlabBlk, + 8 h kCovPitch
    cg = cd = cur_at(s_begin);
  }
  __device__ __forceinline__ Cur cur_at(long long g) const {   // (slab counts fit 31 bits: checked by the launcher)
    Cur c; c.g = g; c.l = (int)((unsigned)g / (unsigned)s_col); c.sc = (int)((unsigned)g - (unsigned)c.l * (unsigned)s_col); return c;
  }
  __device__ __forceinline__ void advance(Cur& c) const { ++c.g; if (++c.sc == s_col) { c.sc = 0; ++c.l; } }
  __device__ __forceinline__ int k0_of(const Cur& c) const { return ((c.sc >> 6) << 10) + ((c.sc & 63) << 3) + gp; }      // subcarrier of half 0; half 1 = + 512
  __device__ __forceinline__ void init(const Cur& c) {
    const int k0 = k0_of(c);
    const bool in = c.g < s_end;
    v_half[0] = in && k0 < K;
    v_half[1] = in && k0 + 512 < K;
    const uint32_t slot = (uint32_t)(((c.sc >> 6) << 9) + ((c.sc & 63) << 3));               // (+ gp: in colbase)
    const uint64_t slab = (uint64_t)slot + (uint64_t)kSpectralSlotsPerColumn * (uint64_t)c.l;   // (scalar registers)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const uint64_t ctr = slab + colbase[j];                         // = (slot + gp) + 2048 (l + L_out ant)
      pc[j][0] = (uint32_t)ctr; pc[j][1] = (uint32_t)(ctr >> 32); pc[j][2] = kSpectralStream; pc[j][3] = 0u;
    }
  }
  template <int R>
  __device__ __forceinline__ void round() {
#pragma unroll
    for (int j = 0; j < 2; ++j) philox4x32_round(pc[j], key0 + (uint32_t)R * 0x9E3779B9u, key1 + (uint32_t)R * 0xBB67AE85u);
  }
  template <int I>                                   // Box-Muller transform I = 2 j + h: antenna set j, half h
  __device__ __forceinline__ void bm() {
    constexpr int j = I / 2, h = I % 2;
    box_muller32_hw_f32(pc[j][2 * h], pc[j][2 * h + 1], wf[j][h][0], wf[j][h][1]);
  }
  template <int I>                                   // synthesis + mask + LDS store of element I = 2 j + h
  __device__ __forceinline__ void emit(const c64 (&dv)[QT][2], c64* img) {
    constexpr int j = I / 2, h = I % 2;
    c64 d[QT];
#pragma unroll
    for (int q = 0; q < QT; ++q) d[q] = dv[q][h];
    c64 v = spectral_echo_value<QT, true>(d, st[j], mk((double)wf[j][h][0], (double)wf[j][h][1]), sig);
    const bool ok = v_half[h] && ant_ok[j];
    v = mk(ok ? v.re : 0.0, ok ? v.im : 0.0);
    img[g_lds0 + 2 * j * kCovSlabBlk + 8 * h * kCovPitch] = v;
  }
  __device__ __forceinline__ void loads(c64 (&dv)[QT][2], const Cur& c) {
    const int k0 = k0_of(c);
    const bool in = c.g < s_end;
    const unsigned base = (unsigned)(((long long)K * c.l + k0) * (long long)sizeof(c64));
    const unsigned o0 = (in && k0 < K) ? base : kCovOobOffset, o1 = (in && k0 + 512 < K) ? base + 512u * (unsigned)sizeof(c64) : kCovOobOffset;
#pragma unroll
    for (int q = 0; q < QT; ++q) { dv[q][0] = buffer_load_c64(rsD[q], o0); dv[q][1] = buffer_load_c64(rsD[q], o1); }
  }
  __device__ __forceinline__ void whole(c64 (&dv)[QT][2], c64* img) {
    loads(dv, cg);
    init(cg);
    static_for<0, 10>([&](auto rc) { round<decltype(rc)::value>(); });
    static_for<0, 4>([&](auto ic) { bm<decltype(ic)::value>(); });
    static_for<0, 4>([&](auto ic) { emit<decltype(ic)::value>(dv, img); });
    advance(cg);
  }
  // slabs 0 and 1 generated outright into images 0 and 1; the D values of slabs 2 and 3 in flight
  __device__ __forceinline__ void prologue(c64* __restrict__ lds) {
    whole(dl[0], lds);
    whole(dl[1], lds + NB * kCovSlabBlk);
    cd = cg;                                         // slab s_begin + 2
    loads(dl[0], cd); advance(cd);
    loads(dl[1], cd); advance(cd);
  }
  __device__ __forceinline__ void begin_step(long long) {}
  template <int PAR, int I>                          // generator piece I of the slab at cursor cg, into image dst
  __device__ __forceinline__ void piece(c64* dst) {
    if constexpr (I == 0) { init(cg); round<0>(); }
    else if constexpr (I < 10) round<I>();
    else if constexpr (I < 14) bm<I - 10>();
    else if constexpr (I < 18) emit<I - 14>(dl[PAR], dst);
    else { loads(dl[PAR], cd); advance(cg); advance(cd); }
  }
  template <int PAR, int K_>
  __device__ __forceinline__ void gap(c64* dst, long long) {
    static_for<0, kLazyPieces>([&](auto ic) {
      if constexpr (lazy_piece_gap(decltype(ic)::value) == K_) piece<PAR, decltype(ic)::value>(dst);
    });
  }
};

template <int QT>
__global__ __launch_bounds__(256, 2) void cov_lazy_kernel(LazyCovArgs a, long long n_slabs, long long slabs_per_wg, double* __restrict__ part /* [gridX][kTiles][2][256] */) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  c64* lds = reinterpret_cast<c64*>(smem_raw);      // [kCovLdsBufs][4 * kCovSlabBlk]
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int grp = wid >> 1, phase = wid & 1;
  const long long s_begin = (long long)blockIdx.x * slabs_per_wg;
  long long s_end = s_begin + slabs_per_wg;
  if (s_end > n_slabs) s_end = n_slabs;
  if (grp == 0) cov_staged_body<4, 0>(CovLazyGenerator<QT>(a, s_begin, s_end), phase, s_begin, s_end, blockIdx.x, part, lds);
  else cov_staged_body<4, 1>(CovLazyGenerator<QT>(a, s_begin, s_end), phase, s_begin, s_end, blockIdx.x, part, lds);
}

// ---------------------------------------------------------------- split lazy covariance: the noise term, with the beam-sum streamed beside it
// With G[n, r] = sum_q a_q[r] d_q[n] + sig w[n, r] (n = (k, l), the lazy echo grid above) the covariance Ra[a, b] = (1/N) sum_n conj(G[n, a]) G[n, b] is
//     N Ra = sig^2 M  +  sig sum_q ( conj(a_q[a]) c_q[b] + conj(c_q[a]) a_q[b] )  +  sum_pq conj(a_p[a]) H_pq a_q[b],
//     M[a, b] = sum_n conj(w[n, a]) w[n, b],   c_q[r] = sum_n w[n, r] conj(d_q[n]),   H_pq = sum_n conj(d_p[n]) d_q[n].
// M is the whole MFMA bulk and depends on the seed and the shape alone -- not on the waveform, D or the steering vectors -- so it can run at the HEAD of the CPI, in the kernel
// that streams txWaveform for the beam-sum: cov_noise_beam_kernel is cov_lazy_kernel with the synthesis taken out of the generator (the UNIT noise value, masked, goes into the
// LDS image; same pair rows, antenna and half masks, and the slab order of that kernel's FULL slabs -- the half slabs, whose partner rows all lie beyond K, are
// cov_noise_tail_kernel's, below -- so the same field elements enter the sum) and the beam-sum's loads and folds in the MFMA gaps instead
// (beam_stream.hpp: the most HBM-bound and the most MFMA-bound kernel of the CPI, each idle in what the other needs, in one instruction stream).  c_q comes from the range
// kernel, which holds w and d in registers (echo_range_xc_kernel, echo.hip; two LoS targets: cov_cross_kernel below); cov_assemble_kernel below puts the three terms together.
struct NoiseBeamArgs {
  const c64* tx;              // [T x A]
  const c64* steer;           // [A x QT] compacted LoS columns on the device, or nullptr: the argument block
  c64* steer_out;             // ctx->steer [2 x A x QT]: written by workgroup 0 when steer == nullptr
  c64* beam;                  // [QT x T]: written inside the BeamWindow's ranges
  long long T;
  unsigned long long seed;
  int K, L_out, A, s_col;     // s_col: FULL slabs per symbol column (noise_walk.hpp)
  BeamWindow bw;
};
constexpr int kBeamSteerPitch = 72;                             // steering image per target: zero from A on (>= kBeamStreamLoads * bs_steps_per_unit(64))
// One unit of a workgroup's walk, relative to `base` (the first sample of the unit's 256, bw_sample): thread i sums sample base + i, or base + i + W when i < d_s (the
// threads in front of the symbol's range take the samples behind its last unit); it owns the sample when d_lo <= i' < d_hi and loads at i' clamped into [c_lo, c_hi].
// An idle entry loads beyond the descriptors and owns nothing.
struct BeamUnitEntry {
  unsigned base16;            // byte offset of sample `base` inside an antenna column (mod 2^32)
  int d_s, d_lo, d_hi, c_lo, c_hi, pad0, pad1;
};
static_assert(sizeof(BeamUnitEntry) == 32, "two 16-byte LDS reads");
__device__ __forceinline__ BeamUnitEntry beam_unit_entry(const BeamWindow& bw, long long k, bool active) {
  BeamUnitEntry e{kCovOobOffset, 0, 0, 0, 0, 0, 0, 0};
  if (!active) return e;
  const int l = (int)(k / bw.units_per_symbol), j = (int)(k - (long long)l * bw.units_per_symbol);
  const long long s = bw_range_start(bw, l), base = bw_floor_line(s) + (long long)j * kBeamUnit;
  long long lo = bw_first(bw, l), hi = bw_range_end(bw, l);
  if (lo < 0) lo = 0;                                           // samples before the waveform have no beam-sum (their coefficient is the zero coef_window_kernel writes)
  const long long span = (long long)(bw.units_per_symbol + 2) * kBeamUnit;
  auto rel = [&](long long x) { const long long d = x - base; return (int)(d < -span ? -span : d > span ? span : d); };
  e.d_s = rel(s);
  if (hi > lo) {
    e.base16 = (unsigned)((unsigned long long)base * sizeof(c64));
    e.d_lo = e.c_lo = rel(lo);
    e.d_hi = rel(hi);
    e.c_hi = rel(hi - 1);
  }
  return e;
}

// box_muller32_hw_f32 (echo_dev.hpp: the same expressions, so an unmasked element has its bits) with the mask applied once, to the radius, in front of the two products
__device__ __forceinline__ void cov_noise_bm_masked(uint32_t ur, uint32_t ua, bool ok, float& re, float& im) {
  const float u = __builtin_fmaf((float)ur, 0x1.0p-32f, 0x1.0p-33f);
  const float rad = __builtin_amdgcn_sqrtf(__builtin_amdgcn_logf(u) * -1.3862943611198906f);
  const float turns = (float)ua * 0x1.0p-32f;
  const float rm = ok ? rad : 0.0f;
  re = rm * __builtin_amdgcn_cosf(turns);
  im = rm * __builtin_amdgcn_sinf(turns);
}

// The slab source of cov_noise_beam_kernel: the unit noise of CovLazyGenerator's slabs (thread -> pair row gp, antennas ga and ga + 32) plus the beam pieces.  Per slab step
// 27 pieces sit in the 30 MFMA gaps: the generator's 18 (counter set-up + 10 Philox rounds, 4 Box-Muller transforms, 4 x (widen + mask + LDS store)) and 9 of the beam-sum --
// two folds of the six values loaded a step ago (antenna order, the additions of beam_sample: the bits beamsum_kernel produces), the store of a finished unit, the running
// unit's offsets, six loads -- interleaved with the generator's first pieces.  The cursors (unit n of the table, step i of the unit) are wave-uniform; nothing branches.
// init / round / advance and the masks are CovLazyGenerator's, restated (that kernel is pinned instruction by instruction; a change there must be made here too); bm is its
// transform with the element's mask on the radius, emit only widens.
template <int QT>
struct CovNoiseBeamSource {
  static constexpr int NB = 4;
  static constexpr int kGaps = 30;
  static constexpr int kPieces = 27;
  struct Cur { int l, sc; long long g; };
  int gp, ga, K, s_col, g_lds0;
  uint32_t key0, key1;
  long long s_end;
  bool ant_ok[2];
  uint64_t colbase[2];
  Cur cg;
  uint32_t pc[2][4];
  float wf[2][2][2];
  bool v_half[2];
  // beam pieces
  int A, spu, W;
  __amdgpu_buffer_rsrc_t rs_tx;                      // the whole waveform [T x A]: the antenna is the load's scalar offset (T A 16 < 2^31: isac_lazy_split_ok)
  unsigned T16, s_ant;                               // bytes of an antenna column; scalar offset of the next load = T16 x its antenna
  int rem;                                           // antennas the running unit has left at the top of step i: A - kBeamStreamLoads i
  __amdgpu_buffer_rsrc_t rs_beam[QT];
  const c64* s_steer;                                // LDS [QT][kBeamSteerPitch]
  const BeamUnitEntry* s_tab;                        // LDS [kBeamStreamTab]
  int n, i, ip;                                      // unit of the table and step of the unit whose loads are issued; step of the loads in flight
  bool fin;                                          // the loads in flight are the last of their unit
  c64 v[kBeamStreamLoads];
  c64 acc[QT];
  unsigned voff, soff;
  __device__ __forceinline__ CovNoiseBeamSource(const NoiseBeamArgs& a, long long s_begin, long long s_end_, const c64* s_steer_, const BeamUnitEntry* s_tab_)
      : gp(threadIdx.x & 7), ga(threadIdx.x >> 3), K(a.K), s_col(a.s_col), key0((uint32_t)a.seed), key1((uint32_t)(a.seed >> 32)), s_end(s_end_), A(a.A),
        spu(bs_steps_per_unit(a.A)), W(a.bw.units_per_symbol * kBeamUnit), rs_tx(buffer_of(a.tx, (unsigned)(a.T * (long long)a.A * (long long)sizeof(c64)))),
        T16(__builtin_amdgcn_readfirstlane((unsigned)(a.T * (long long)sizeof(c64)))), s_ant(0u), rem(a.A), s_steer(s_steer_), s_tab(s_tab_), n(0), i(0), ip(0), fin(false), voff(kCovOobOffset), soff(kCovOobOffset) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ant = ga + 32 * j;
      ant_ok[j] = ant < a.A;
      colbase[j] = (uint64_t)gp + (uint64_t)kSpectralSlotsPerColumn * ((uint64_t)a.L_out * (uint64_t)ant);
    }
    g_lds0 = (ga >> 4) * kCovSlabBlk + gp * kCovPitch + ((ga & 15) ^ kCovSwizzle(gp));
    Cur c; c.g = s_begin; c.l = (int)((unsigned)s_begin / (unsigned)s_col); c.sc = (int)((unsigned)s_begin - (unsigned)c.l * (unsigned)s_col);
    cg = c;
#pragma unroll
    for (int q = 0; q < QT; ++q) { rs_beam[q] = buffer_of(a.beam + (long long)q * a.T, (unsigned)(a.T * (long long)sizeof(c64))); acc[q] = mk(0.0, 0.0); }
#pragma unroll
    for (int j = 0; j < kBeamStreamLoads; ++j) v[j] = mk(0.0, 0.0);
  }
  __device__ __forceinline__ void advance(Cur& c) const { ++c.g; if (++c.sc == s_col) { c.sc = 0; ++c.l; } }
  __device__ __forceinline__ void init(const Cur& c) {          // (CovLazyGenerator::init)
    const int k0 = ((c.sc >> 6) << 10) + ((c.sc & 63) << 3) + gp;
    const bool in = c.g < s_end;
    v_half[0] = in && k0 < K;
    v_half[1] = in && k0 + 512 < K;
    const uint32_t slot = (uint32_t)(((c.sc >> 6) << 9) + ((c.sc & 63) << 3));
    const uint64_t slab = (uint64_t)slot + (uint64_t)kSpectralSlotsPerColumn * (uint64_t)c.l;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const uint64_t ctr = slab + colbase[j];
      pc[j][0] = (uint32_t)ctr; pc[j][1] = (uint32_t)(ctr >> 32); pc[j][2] = kSpectralStream; pc[j][3] = 0u;
    }
  }
  template <int R>
  __device__ __forceinline__ void round() {
#pragma unroll
    for (int j = 0; j < 2; ++j) philox4x32_round(pc[j], key0 + (uint32_t)R * 0x9E3779B9u, key1 + (uint32_t)R * 0xBB67AE85u);
  }
  template <int I>                                   // box_muller32_hw_f32 with the element's mask on the radius: a masked element is (+-0, +-0), which changes no sum
  __device__ __forceinline__ void bm() {
    constexpr int j = I / 2, h = I % 2;
    cov_noise_bm_masked(pc[j][2 * h], pc[j][2 * h + 1], v_half[h] && ant_ok[j], wf[j][h][0], wf[j][h][1]);
  }
  template <int I>                                   // widen + LDS store of unit noise element I = 2 j + h (masked in bm)
  __device__ __forceinline__ void emit(c64* img) {
    constexpr int j = I / 2, h = I % 2;
    img[g_lds0 + 2 * j * kCovSlabBlk + 8 * h * kCovPitch] = mk((double)wf[j][h][0], (double)wf[j][h][1]);
  }
  template <int I>                                   // generator piece I of the slab at cursor cg, into image dst
  __device__ __forceinline__ void gen(c64* dst) {
    if constexpr (I == 0) { init(cg); round<0>(); }
    else if constexpr (I < 10) round<I>();
    else if constexpr (I < 14) bm<I - 10>();
    else { emit<I - 14>(dst); if constexpr (I == 17) advance(cg); }
  }
  __device__ __forceinline__ void whole(c64* img) {
    static_for<0, 18>([&](auto ic) { gen<decltype(ic)::value>(img); });
  }
  __device__ __forceinline__ void prologue(c64* __restrict__ lds) {   // slabs 0 and 1 generated outright into images 0 and 1
    whole(lds);
    whole(lds + NB * kCovSlabBlk);
  }
  __device__ __forceinline__ void begin_step(long long) {}
  template <int J0>
  __device__ __forceinline__ void fold() {           // values J0 .. J0 + 2 of the loads in flight, in antenna order
    const c64* sp = s_steer + ip * kBeamStreamLoads;
#pragma unroll
    for (int j = J0; j < J0 + kBeamStreamLoads / 2; ++j)
#pragma unroll
      for (int q = 0; q < QT; ++q) acc[q] = fma(v[j], sp[q * kBeamSteerPitch + j], acc[q]);
  }
  __device__ __forceinline__ void finish() {         // behind the last fold of a unit: its sums go out (a store beyond the descriptor is dropped), the next unit starts from zero
    const unsigned so = fin ? soff : kCovOobOffset;
#pragma unroll
    for (int q = 0; q < QT; ++q) {
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, acc[q]), rs_beam[q], (int)so, 0, 0);
      acc[q] = mk(fin ? 0.0 : acc[q].re, fin ? 0.0 : acc[q].im);
    }
  }
  __device__ __forceinline__ void offsets() {        // this thread's sample of unit n
    const uint4 e0 = *reinterpret_cast<const uint4*>(s_tab + n);
    const uint4 e1 = *(reinterpret_cast<const uint4*>(s_tab + n) + 1);
    const int tid = threadIdx.x;
    const int ur = tid + (tid < (int)e0.y ? W : 0);
    const bool mine = ur >= (int)e0.z && ur < (int)e0.w;
    int uc = ur < (int)e1.x ? (int)e1.x : ur;
    uc = uc > (int)e1.y ? (int)e1.y : uc;
    voff = e0.x + (unsigned)uc * (unsigned)sizeof(c64);
    soff = mine ? voff : kCovOobOffset;
  }
  template <int J>
  __device__ __forceinline__ void load() {           // antenna slot J of step i
    // (wave-uniform) antenna bs_antenna(i, J) = slot J of the rem left: a padding slot loads beyond the descriptor -- a true zero, whatever the waveform holds.  voff stays
    // inside the antenna's column, so voff + s_ant is inside the descriptor; the antennas of a step ascend, the scalar offset moves on by a column per load.
    v[J] = __builtin_bit_cast(c64, __builtin_amdgcn_raw_buffer_load_b128(rs_tx, (int)(J < rem ? voff : kCovOobOffset), (int)s_ant, 0));
    s_ant += T16;
    if constexpr (J == kBeamStreamLoads - 1) {
      const bool last = i == spu - 1;
      ip = i;
      fin = last;
      i = last ? 0 : i + 1;
      s_ant = last ? 0u : s_ant;
      rem = last ? A : rem - kBeamStreamLoads;
      n = (last && n < kBeamStreamTab - 1) ? n + 1 : n;
    }
  }
  template <int I>
  __device__ __forceinline__ void beam() {
    if constexpr (I == 0) fold<0>();
    else if constexpr (I == 1) { fold<kBeamStreamLoads / 2>(); finish(); }
    else if constexpr (I == 2) offsets();
    else load<I - 3>();
  }
  // piece P of a step: the first 18 alternate generator / beam, the last 9 are the generator's
  template <int P>
  __device__ __forceinline__ void piece(c64* dst) {
    if constexpr (P >= 18) gen<P - 9>(dst);
    else if constexpr (P % 2 == 0) gen<P / 2>(dst);
    else beam<P / 2>();
  }
  static __host__ __device__ constexpr int piece_gap(int p) { return (p * 30) / kPieces; }
  template <int PAR, int K_>
  __device__ __forceinline__ void gap(c64* dst, long long) {
    static_for<0, kPieces>([&](auto ic) {
      if constexpr (piece_gap(decltype(ic)::value) == K_) piece<decltype(ic)::value>(dst);
    });
  }
};

template <int QT>
__global__ __launch_bounds__(256, 2) void cov_noise_beam_kernel(NoiseBeamArgs a, const SteerArg steer_arg, long long n_slabs, long long slabs_per_wg,
                                                                double* __restrict__ part /* [gridX][kTiles][2][256] */) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  c64* lds = reinterpret_cast<c64*>(smem_raw);      // [kCovLdsBufs][4 * kCovSlabBlk] | steering image [QT][kBeamSteerPitch] | unit table [kBeamStreamTab]
  c64* s_steer = lds + kCovLdsBufs * 4 * kCovSlabBlk;
  BeamUnitEntry* s_tab = reinterpret_cast<BeamUnitEntry*>(s_steer + QT * kBeamSteerPitch);
  const int tid = threadIdx.x;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wid >> 1, phase = wid & 1;
  const int A = a.A, wg = blockIdx.x, n_wg = gridDim.x;
  const long long s_begin = (long long)wg * slabs_per_wg;
  long long s_end = s_begin + slabs_per_wg;
  if (s_end > n_slabs) s_end = n_slabs;
  const int my_units = bs_units_of(bw_units(a.bw), n_wg, wg);
  const int n_stream = bs_stream_units(my_units, bs_steps_of(n_slabs, slabs_per_wg, wg), bs_steps_per_unit(A));
  for (int i = tid; i < QT * kBeamSteerPitch; i += 256) {
    const int q = i / kBeamSteerPitch, r = i - q * kBeamSteerPitch;
    c64 sv = mk(0.0, 0.0);
    if (r < A) {
      sv = a.steer ? a.steer[q * A + r] : steer_arg.v[q * A + r];
      if (!a.steer && wg == 0) {
        a.steer_out[q * A + r] = sv;
        a.steer_out[A * QT + r * QT + q] = sv;       // row r of the transpose holds a_q[r] at r QT + q
      }
    }
    s_steer[i] = sv;
  }
  if (tid < kBeamStreamTab) s_tab[tid] = beam_unit_entry(a.bw, bs_unit(n_wg, wg, tid), tid < n_stream);
  __syncthreads();
  if (grp == 0) cov_staged_body<4, 0>(CovNoiseBeamSource<QT>(a, s_begin, s_end, s_steer, s_tab), phase, s_begin, s_end, wg, part, lds);
  else cov_staged_body<4, 1>(CovNoiseBeamSource<QT>(a, s_begin, s_end, s_steer, s_tab), phase, s_begin, s_end, wg, part, lds);
  // the units the slab steps did not reach (small K against a full waveform): beamsum_coef_kernel's walk, sums only
  for (int t = n_stream; t < my_units; ++t) {
    const long long k = bs_unit(n_wg, wg, t);
    const int l = (int)(k / a.bw.units_per_symbol), j = (int)(k - (long long)l * a.bw.units_per_symbol);
    const long long lo = bw_first(a.bw, l), hi = bw_range_end(a.bw, l);
    const long long u = bw_sample(a.bw, l, j, tid);
    const bool mine = u >= lo && u < hi;
    if (!__any(mine)) continue;                      // (wave-uniform; no barrier in this loop)
    long long uc = u < lo ? lo : u < hi ? u : hi - 1;
    uc = uc < 0 ? 0 : uc < a.T ? uc : a.T - 1;
    const c64* p = a.tx + uc;
    c64 acc[QT];
#pragma unroll
    for (int q = 0; q < QT; ++q) acc[q] = mk(0.0, 0.0);
    constexpr int UN = 16;
    int r = 0;
    for (; r + UN <= A; r += UN) {
      c64 vv[UN];
#pragma unroll
      for (int x = 0; x < UN; ++x) vv[x] = p[(long long)(r + x) * a.T];
#pragma unroll
      for (int x = 0; x < UN; ++x)
#pragma unroll
        for (int q = 0; q < QT; ++q) acc[q] = fma(vv[x], s_steer[q * kBeamSteerPitch + r + x], acc[q]);
    }
    for (; r < A; ++r) {
      const c64 vv = p[(long long)r * a.T];
#pragma unroll
      for (int q = 0; q < QT; ++q) acc[q] = fma(vv, s_steer[q * kBeamSteerPitch + r], acc[q]);
    }
    if (mine && u >= 0) {
#pragma unroll
      for (int q = 0; q < QT; ++q) a.beam[(long long)q * a.T + u] = acc[q];
    }
  }
}

// ---------------------------------------------------------------- the half slabs of the noise term, packed two to a slab (noise_walk.hpp)
// Where K is no multiple of 1024 the last block pair of every symbol column has rows whose partner k + 512 lies beyond K: slabs whose sample slots 8..15 are all masked, a
// full step each in the regenerating route's walk (26 of 218 per column at K = 3276).  cov_noise_beam_kernel walks the full slabs alone; cov_noise_tail_kernel forms the half
// slabs two to a slab -- sample slots 0..7 the first halves of one Philox slot group, 8..15 those of another: four calls per thread and step, outputs 0-1 of each -- so the
// same field elements enter M in half the steps; only their order in the sum changes.  It carries no beam-sum, appends its partials behind the main kernel's and runs off the
// CPI's serial chain (isac_cov_noise_beam_on).
struct NoiseTailArgs {
  unsigned long long seed;
  int K, L_out, A;
  NoiseWalk w;
};

// The slab source of cov_noise_tail_kernel: thread -> (row gp of both half slabs, antennas ga and ga + 32).  18 pieces per step (counter set-up + 10 Philox rounds of the four
// calls, 4 Box-Muller transforms, 4 x (widen + LDS store)), spread over the 30 MFMA gaps.  Counter, masks and transform as in CovNoiseBeamSource.
struct CovNoiseTailSource {
  static constexpr int NB = 4;
  static constexpr int kGaps = 30;
  static constexpr int kPieces = 18;
  struct Cur { int l, u; long long g; };             // packed slab g = packed slab u of symbol column l
  int gp, ga, K, g_lds0;
  NoiseWalk w;
  uint32_t key0, key1;
  long long s_end;
  bool ant_ok[2];
  uint64_t colbase[2];
  Cur cg;
  uint32_t pc[2][2][4];                              // [antenna set j][half h]
  float wf[2][2][2];
  bool v_half[2];
  __device__ __forceinline__ CovNoiseTailSource(const NoiseTailArgs& a, long long s_begin, long long s_end_)
      : gp(threadIdx.x & 7), ga(threadIdx.x >> 3), K(a.K), w(a.w), key0((uint32_t)a.seed), key1((uint32_t)(a.seed >> 32)), s_end(s_end_) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ant = ga + 32 * j;
      ant_ok[j] = ant < a.A;
      colbase[j] = (uint64_t)gp + (uint64_t)kSpectralSlotsPerColumn * ((uint64_t)a.L_out * (uint64_t)ant);
    }
    g_lds0 = (ga >> 4) * kCovSlabBlk + gp * kCovPitch + ((ga & 15) ^ kCovSwizzle(gp));
    Cur c; c.g = s_begin; c.l = (int)((unsigned)s_begin / (unsigned)w.n_packed); c.u = (int)((unsigned)s_begin - (unsigned)c.l * (unsigned)w.n_packed);   // (n_packed >= 1: the launcher)
    cg = c;
  }
  __device__ __forceinline__ void advance(Cur& c) const { ++c.g; if (++c.u == w.n_packed) { c.u = 0; ++c.l; } }
  __device__ __forceinline__ void init(const Cur& c) {
    const bool in = c.g < s_end;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      v_half[h] = in && nw_tail_has(w, c.u, h) && nw_tail_row(w, c.u, h, gp) < K;
      const uint64_t slab = (uint64_t)(uint32_t)nw_tail_slot(w, c.u, h, 0) + (uint64_t)kSpectralSlotsPerColumn * (uint64_t)c.l;   // (+ gp: in colbase)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const uint64_t ctr = slab + colbase[j];
        pc[j][h][0] = (uint32_t)ctr; pc[j][h][1] = (uint32_t)(ctr >> 32); pc[j][h][2] = kSpectralStream; pc[j][h][3] = 0u;
      }
    }
  }
  template <int R>
  __device__ __forceinline__ void round() {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int h = 0; h < 2; ++h) philox4x32_round(pc[j][h], key0 + (uint32_t)R * 0x9E3779B9u, key1 + (uint32_t)R * 0xBB67AE85u);
  }
  template <int I>                                   // element I = 2 j + h: outputs 0-1 of its call, masked on the radius
  __device__ __forceinline__ void bm() {
    constexpr int j = I / 2, h = I % 2;
    cov_noise_bm_masked(pc[j][h][0], pc[j][h][1], v_half[h] && ant_ok[j], wf[j][h][0], wf[j][h][1]);
  }
  template <int I>
  __device__ __forceinline__ void emit(c64* img) {
    constexpr int j = I / 2, h = I % 2;
    img[g_lds0 + 2 * j * kCovSlabBlk + 8 * h * kCovPitch] = mk((double)wf[j][h][0], (double)wf[j][h][1]);
  }
  template <int I>
  __device__ __forceinline__ void gen(c64* dst) {
    if constexpr (I == 0) { init(cg); round<0>(); }
    else if constexpr (I < 10) round<I>();
    else if constexpr (I < 14) bm<I - 10>();
    else { emit<I - 14>(dst); if constexpr (I == 17) advance(cg); }
  }
  __device__ __forceinline__ void whole(c64* img) {
    static_for<0, kPieces>([&](auto ic) { gen<decltype(ic)::value>(img); });
  }
  __device__ __forceinline__ void prologue(c64* __restrict__ lds) {
    whole(lds);
    whole(lds + NB * kCovSlabBlk);
  }
  __device__ __forceinline__ void begin_step(long long) {}
  static __host__ __device__ constexpr int piece_gap(int p) { return (p * 30) / kPieces; }
  template <int PAR, int K_>
  __device__ __forceinline__ void gap(c64* dst, long long) {
    static_for<0, kPieces>([&](auto ic) {
      if constexpr (piece_gap(decltype(ic)::value) == K_) gen<decltype(ic)::value>(dst);
    });
  }
};

__global__ __launch_bounds__(256, 2) void cov_noise_tail_kernel(NoiseTailArgs a, long long n_slabs, long long slabs_per_wg, int part0,
                                                                double* __restrict__ part /* [part0 + gridX][kTiles][2][256] */) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  c64* lds = reinterpret_cast<c64*>(smem_raw);      // [kCovLdsBufs][4 * kCovSlabBlk]
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int grp = wid >> 1, phase = wid & 1;
  const long long s_begin = (long long)blockIdx.x * slabs_per_wg;
  long long s_end = s_begin + slabs_per_wg;
  if (s_end > n_slabs) s_end = n_slabs;
  if (grp == 0) cov_staged_body<4, 0>(CovNoiseTailSource(a, s_begin, s_end), phase, s_begin, s_end, part0 + (int)blockIdx.x, part, lds);
  else cov_staged_body<4, 1>(CovNoiseTailSource(a, s_begin, s_end), phase, s_begin, s_end, part0 + (int)blockIdx.x, part, lds);
}

// The cross term where the range kernel cannot carry it (two LoS targets: echo_range_sl_kernel<2, 1, false, 2> sits at exactly 128 registers, echo.hip): a pass of its own over
// w and D, in fft2D, off the serial chain of the CPI.  One workgroup per column (l, r); thread tid draws the column's Philox calls tid + 256 c -- slot s serves the rows
// k0 = (s mod 512) + 1024 (s div 512) and k0 + 512, counter s + 2048 (l + L_out r): the field of echo_dev.hpp, box_muller32_hw's bits -- and sums w conj(d_q) over k < K;
// the workgroup's sums are added in a fixed-order tree.  xc[(l A + r) QT + q], the layout echo_range_xc_kernel writes.
template <int QT>
__global__ __launch_bounds__(256) void cov_cross_kernel(const c64* __restrict__ D /* [K x L x QT] */, int K, int L, int L_out, int A, unsigned long long seed,
                                                        c64* __restrict__ xc /* [L][A][QT] */) {
  __shared__ c64 s_sum[QT][256];
  const int l = blockIdx.x % L, r = blockIdx.x / L, tid = threadIdx.x;
  const unsigned long long colg = (unsigned long long)l + (unsigned long long)L_out * (unsigned long long)r;
  c64 acc[QT];
#pragma unroll
  for (int q = 0; q < QT; ++q) acc[q] = mk(0.0, 0.0);
  for (int s = tid; s < kSpectralSlotsPerColumn; s += 256) {
    const int k0 = (s & 511) + ((s >> 9) << 10);
    if (k0 >= K) break;                              // (k0 grows with s)
    const uint64_t ctr = (uint64_t)s + (uint64_t)kSpectralSlotsPerColumn * colg;
    uint32_t o[4];
    philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), kSpectralStream, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), o);
    const c64 w0 = box_muller32_hw(o[0], o[1]);
#pragma unroll
    for (int q = 0; q < QT; ++q) acc[q] = fma(w0, conj(D[(long long)K * ((long long)l + (long long)L * q) + k0]), acc[q]);
    if (k0 + 512 < K) {
      const c64 w1 = box_muller32_hw(o[2], o[3]);
#pragma unroll
      for (int q = 0; q < QT; ++q) acc[q] = fma(w1, conj(D[(long long)K * ((long long)l + (long long)L * q) + k0 + 512]), acc[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < QT; ++q) s_sum[q][tid] = acc[q];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) {
#pragma unroll
      for (int q = 0; q < QT; ++q) s_sum[q][tid] += s_sum[q][tid + w];
    }
    __syncthreads();
  }
  if (tid < QT) xc[((long long)l * A + r) * QT + tid] = s_sum[tid][0];
}

// H[l][p][q] = sum_k conj(d_p[k, l]) d_q[k, l]: one workgroup per symbol column, a fixed-order tree
template <int QT>
__global__ __launch_bounds__(256) void cov_dgram_kernel(const c64* __restrict__ D /* [K x L x QT] */, int K, int L, c64* __restrict__ H /* [L][QT][QT] */) {
  __shared__ c64 s_sum[256];
  const int l = blockIdx.x, tid = threadIdx.x;
#pragma unroll
  for (int p = 0; p < QT; ++p)
#pragma unroll
    for (int q = 0; q < QT; ++q) {
      const c64 *dp = D + (long long)K * ((long long)l + (long long)L * p), *dq = D + (long long)K * ((long long)l + (long long)L * q);
      c64 s = mk(0.0, 0.0);
      for (int k = tid; k < K; k += 256) s = fma(conj(dp[k]), dq[k], s);
      __syncthreads();
      s_sum[tid] = s;
      __syncthreads();
      for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) s_sum[tid] += s_sum[tid + w];
        __syncthreads();
      }
      if (tid == 0) H[((long long)l * QT + p) * QT + q] = s_sum[0];
    }
}

// Ra = sig^2 (M / N) + ( sig sum_q (conj(a_q[a]) c_q[b] + conj(c_q[a]) a_q[b]) + sum_pq conj(a_p[a]) H_pq a_q[b] ) / N   (the split above).  One workgroup: the cross
// partials xc[l][r][q] (echo_range_xc_kernel) and H[l] are summed over the symbols in index order; the upper triangle is computed and mirrored by conjugation, the diagonal's
// imaginary part is set to zero -- exactly Hermitian, as cov_reduce_kernel leaves it.
template <int QT>
__global__ __launch_bounds__(256) void cov_assemble_kernel(const c64* __restrict__ Mn /* [A x A] = M / N */, const c64* __restrict__ xc /* [L][A][QT] */,
                                                           const c64* __restrict__ H /* [L][QT][QT] */, const c64* __restrict__ steer_rq /* [A x QT]: a_q[r] at r QT + q */,
                                                           int A, int L, double sig, double inv_n, c64* __restrict__ Ra) {
  __shared__ c64 s_c[64 * QT], s_a[64 * QT], s_h[QT * QT], s_p[256];
  const int tid = threadIdx.x;
  // the symbol sums in kParts interleaved runs per entry (l = p, p + kParts, ...: independent loads, eight in flight), the runs then added in the order of p
  constexpr int kParts = 256 / (64 * QT);
  {
    const int i = tid % (64 * QT), p = tid / (64 * QT);
    c64 s = mk(0.0, 0.0);
    if (i < A * QT) {
#pragma unroll 8
      for (int l = p; l < L; l += kParts) s += xc[(long long)l * A * QT + i];
    }
    s_p[tid] = s;
  }
  __syncthreads();
  for (int i = tid; i < A * QT; i += 256) {
    c64 s = s_p[i];
#pragma unroll
    for (int p = 1; p < kParts; ++p) s += s_p[p * 64 * QT + i];
    s_c[i] = s;
    s_a[i] = steer_rq[i];
  }
  if (tid >= 128 && tid < 128 + QT * QT) {
    c64 s = mk(0.0, 0.0);
#pragma unroll 8
    for (int l = 0; l < L; ++l) s += H[(long long)l * QT * QT + (tid - 128)];
    s_h[tid - 128] = s;
  }
  __syncthreads();
  for (int e = tid; e < A * A; e += 256) {
    const int a = e % A, b = e / A;
    if (a > b) continue;
    c64 x = mk(0.0, 0.0), h = mk(0.0, 0.0);
#pragma unroll
    for (int q = 0; q < QT; ++q) {
      x = fma(conj(s_a[a * QT + q]), s_c[b * QT + q], x);
      x = fma(conj(s_c[a * QT + q]), s_a[b * QT + q], x);
      c64 hq = mk(0.0, 0.0);                          // sum_p conj(a_p[a]) H_pq
#pragma unroll
      for (int p = 0; p < QT; ++p) hq = fma(conj(s_a[a * QT + p]), s_h[p * QT + q], hq);
      h = fma(hq, s_a[b * QT + q], h);
    }
    const c64 m = Mn[a + (long long)A * b];
    c64 v = mk(::fma(sig * sig, m.re, (sig * x.re + h.re) * inv_n), ::fma(sig * sig, m.im, (sig * x.im + h.im) * inv_n));
    if (a == b) v.im = 0.0;
    Ra[a + (long long)A * b] = v;
    if (a != b) Ra[b + (long long)A * a] = conj(v);
  }
}

__global__ __launch_bounds__(256, 2) void cov_mfma_block_kernel(const c64* __restrict__ G, long long N, int A, int n_blk,
                                                                int n_pairs, long long slabs_per_wg,
                                                                double* __restrict__ part /* [chunk][pair][16][2][256] */) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  c64* lds = reinterpret_cast<c64*>(smem_raw);      // [2][kCovBufElems]
  // (pinning the block pairs of one sample chunk to one XCD -- workgroup b runs on XCD b % 8 -- so that a chunk's slabs enter ONE L2: 3.71 ->
  // 4.11 ms at A = 256, no change at A = 128: the diagonal pairs run 1.6x faster than the off-diagonal ones and drift out of the L2 window)
  const int pair = blockIdx.x % n_pairs, chunk = blockIdx.x / n_pairs;
  int BI, BJ;
  cov_pair_blocks(n_blk, pair, BI, BJ);
  if (BI == BJ) cov_block_pair<true>(G, N, A, BI, BJ, pair, chunk, n_pairs, slabs_per_wg, part, lds);
  else cov_block_pair<false>(G, N, A, BI, BJ, pair, chunk, n_pairs, slabs_per_wg, part, lds);
}

// fixed-order sum over the sample chunks of one tile + Hermitian fill + 1/N (block layout of cov_mfma_block_kernel)
__global__ __launch_bounds__(1024) void cov_block_reduce_kernel(const double* __restrict__ part, int n_chunks, int n_blk, int n_pairs,
                                                                int A, double inv_n, c64* __restrict__ Ra) {
  __shared__ double s_sum[2][4][256];
  const int tile = blockIdx.x, pair = blockIdx.y;
  int BI, BJ;
  cov_pair_blocks(n_blk, pair, BI, BJ);
  const int I = tile >> 2, J = tile & 3;
  if (BI == BJ && J < I) return;                    // never computed
  const int e = threadIdx.x, g = threadIdx.y;
  const int per = (n_chunks + 3) / 4;
  const int c0 = g * per, c1 = min(n_chunks, c0 + per);
  double sr = 0.0, si = 0.0;
  for (int c = c0; c < c1; ++c) {
    const double* o = part + ((((long long)c * n_pairs + pair) * 16 + tile) * 2) * 256;
    sr += o[e];
    si += o[256 + e];
  }
  s_sum[0][g][e] = sr; s_sum[1][g][e] = si;
  __syncthreads();
  if (g != 0) return;
  sr = ((s_sum[0][0][e] + s_sum[0][1][e]) + s_sum[0][2][e]) + s_sum[0][3][e];
  si = ((s_sum[1][0][e] + s_sum[1][1][e]) + s_sum[1][2][e]) + s_sum[1][3][e];
  const int r = e >> 6, lane = e & 63;
  if (BI == BJ && I == J) {                         // diagonal tile: the partials hold M, Im = M - M^T
    const int row = (lane >> 4) + 4 * r, col = lane & 15;
    const int et = (col >> 2) * 64 + ((col & 3) << 4) + row;
    si -= ((s_sum[1][0][et] + s_sum[1][1][et]) + s_sum[1][2][et]) + s_sum[1][3][et];
  }
  const int a = 64 * BI + 16 * I + (lane >> 4) + 4 * r;   // f64 MFMA C/D layout: row = (lane>>4) + 4*reg, col = lane&15
  const int b = 64 * BJ + 16 * J + (lane & 15);
  if (a >= A || b >= A) return;
  c64 v = mk(sr * inv_n, si * inv_n);
  if (a == b) v.im = 0.0;
  if (BI == BJ && I == J && a > b) return;          // diagonal tile: keep the upper triangle, mirror it (exactly Hermitian)
  Ra[a + (long long)A * b] = v;
  if (a != b) Ra[b + (long long)A * a] = conj(v);
}

// first reduction level: slice s of S sums a contiguous run of workgroup partials (fixed order) into part2[s];
// spreads the 60 MB of partial tiles over S x n_tiles workgroups instead of n_tiles (per-CU bandwidth bound)
__global__ __launch_bounds__(256) void cov_reduce_slice_kernel(const double* __restrict__ part, int n_wg, int n_tiles, int S,
                                                               double* __restrict__ part2 /* [S][n_tiles][2][256] */) {
  const int t = blockIdx.x, sl = blockIdx.y, e = threadIdx.x;
  const int per = (n_wg + S - 1) / S;
  const int w0 = sl * per, w1 = min(n_wg, w0 + per);
  double sr = 0.0, si = 0.0;
#pragma unroll 8
  for (int w = w0; w < w1; ++w) {
    const double* o = part + (((long long)w * n_tiles + t) * 2) * 256;
    sr += o[e];
    si += o[256 + e];
  }
  double* d = part2 + (((long long)sl * n_tiles + t) * 2) * 256;
  d[e] = sr; d[256 + e] = si;
}

// fixed-order reduction over workgroup partials + Hermitian fill + 1/N.
__global__ __launch_bounds__(1024) void cov_reduce_kernel(const double* __restrict__ part, int n_wg, int n_tiles, int A,
                                                          double inv_n, c64* __restrict__ Ra /* [A x A] column-major */) {
  __shared__ double s_sum[2][4][256];
  const int t = blockIdx.x;
  const int nb = (A + 15) / 16;
  const int I = cov_tile_i(nb, t), J = cov_tile_j(nb, t);
  const int e = threadIdx.x;            // r*64 + lane
  const int g = threadIdx.y;
  const int r = e >> 6, lane = e & 63;
  const int row = (lane >> 4) + 4 * r;  // f64 MFMA C/D layout: row = (lane>>4) + 4*reg, col = lane&15
  const int col = lane & 15;
  const int per = (n_wg + 3) / 4;
  const int w0 = g * per, w1 = min(n_wg, w0 + per);
  double sr = 0.0, si = 0.0;
#pragma unroll 8
  for (int w = w0; w < w1; ++w) {
    const double* o = part + (((long long)w * n_tiles + t) * 2) * 256;
    sr += o[e];
    si += o[256 + e];
  }
  s_sum[0][g][e] = sr; s_sum[1][g][e] = si;
  __syncthreads();
  if (g != 0) return;
  sr = ((s_sum[0][0][e] + s_sum[0][1][e]) + s_sum[0][2][e]) + s_sum[0][3][e];
  si = ((s_sum[1][0][e] + s_sum[1][1][e]) + s_sum[1][2][e]) + s_sum[1][3][e];
  if (I == J) {                                                       // diagonal tiles hold M: Im = M - M^T
    const int et = (col >> 2) * 64 + ((col & 3) << 4) + row;          // the (col, row) entry of the same tile
    si -= ((s_sum[1][0][et] + s_sum[1][1][et]) + s_sum[1][2][et]) + s_sum[1][3][et];
  }
  const int a = I * 16 + row, b = J * 16 + col;
  if (a < A && b < A) {
    c64 v = mk(sr * inv_n, si * inv_n);
    if (I == J) {
      if (a == b) v.im = 0.0;
      // both triangles of a diagonal tile are computed; keep the upper one and mirror it so
      // the matrix is exactly Hermitian (zherk-like), as MATLAB's X*X' is
      if (a <= b) {
        Ra[a + (long long)A * b] = v;
        if (a != b) Ra[b + (long long)A * a] = conj(v);
      }
    } else {
      Ra[a + (long long)A * b] = v;
      Ra[b + (long long)A * a] = conj(v);
    }
  }
}

}  // namespace isac

// ================================================================= host side
using namespace isac;

extern "C" int isac_covariance_dev(isac_ctx* ctx, const isac_c64* d_grid, int64_t N, int32_t A, isac_c64* d_Ra) {
  ISAC_ENTER(ctx);
  return isac_covariance_on(ctx, ctx->stream, d_grid, N, A, d_Ra);
}
// isac_profile_enable(ctx, 2): HIP events around exactly the wide covariance launch (bench.py's roofline entry when that launch is the longest of the CPI)
#define ISAC_PROF_COV0(st) do { if (ctx->profile_cov) ISAC_HIP(hipEventRecord(ctx->ev_k0, st)); } while (0)
#define ISAC_PROF_COV1(st) do { if (ctx->profile_cov) { ISAC_HIP(hipEventRecord(ctx->ev_k1, st)); ctx->profile_recorded = true; } } while (0)
// Grid of a staged launch (cov_mfma_lds_kernel, cov_lazy_kernel) over `slabs` slabs: at most 512 workgroups (2 per CU: register-limited occupancy), each
// walking `per` slabs, in pairs.
static void cov_staged_grid(long long slabs, long long& gx, long long& per) {
  gx = 512 < slabs ? 512 : slabs;
  per = (slabs + gx - 1) / gx;
  per = (per + 1) & ~1ll;
  gx = (slabs + per - 1) / per;
}

// Sizes cov_part for n_part workgroup partials [n_part][n_tiles][2][256] (+ the 32 slices of the first reduction level), has `launch(part)` enqueue the kernel
// that writes them, and enqueues the two-level fixed-order reduction into Ra.
template <class Launch>
static int cov_partials_to_ra(isac_ctx* ctx, hipStream_t st, int n_part, int n_tiles, int A, double inv_n, c64* Ra, Launch&& launch) {
  const int S = 32;
  ISAC_TRY(ensure(ctx, ctx->cov_part, sizeof(double) * ((size_t)n_part + S) * n_tiles * 2 * 256));
  double* part = (double*)ctx->cov_part.p;
  double* part2 = part + (size_t)n_part * n_tiles * 2 * 256;
  ISAC_TRY(launch(part));
  hipLaunchKernelGGL(cov_reduce_slice_kernel, dim3(n_tiles, S), dim3(256), 0, st, (const double*)part, n_part, n_tiles, S, part2);
  ISAC_HIP(hipGetLastError());
  hipLaunchKernelGGL(cov_reduce_kernel, dim3(n_tiles), dim3(256, 4), 0, st, (const double*)part2, S, n_tiles, A, inv_n, Ra);
  ISAC_HIP(hipGetLastError());
  return ISAC_OK;
}

template <int NB>
static int launch_cov_small(isac_ctx* ctx, hipStream_t st, const c64* G, long long N, int A, c64* Ra) {
  using P = CovPlan<NB>;
  const long long total = (N + 15) / 16;
  if (N * 256 >= (1ll << 32)) return fail(ctx, ISAC_ERR_UNSUPPORTED, "covariance: at most 2^24 - 1 samples per antenna");
  const bool staged = (NB >= 3) && N * 256 < (1ll << 31);           // two tile groups: fetch each slab once per workgroup, through LDS
  long long gx, per;
  if (staged) {
    cov_staged_grid(total, gx, per);
  } else {
    gx = NB == 4 ? 512 : 768;                 // NB = 4: 2 workgroups per CU (register-limited occupancy)
    if (gx > total) gx = total;
    per = (total + gx - 1) / gx;
    gx = (total + per - 1) / per;
  }
  const int n_part = (int)gx * (staged ? 1 : P::kPhases);       // (the staged kernel sums its two sample phases itself)
  return cov_partials_to_ra(ctx, st, n_part, P::kTiles, A, 1.0 / (double)N, Ra, [&](double* part) -> int {
    if constexpr (NB >= 3) {
      if (staged) {
        const size_t lds = sizeof(c64) * kCovLdsBufs * NB * kCovSlabBlk;
        ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(cov_mfma_lds_kernel<NB>), lds));
        ISAC_PROF_COV0(st);
        hipLaunchKernelGGL((cov_mfma_lds_kernel<NB>), dim3((unsigned)gx), dim3(256), lds, st, G, N, A, per, part);
        ISAC_HIP(hipGetLastError());
        ISAC_PROF_COV1(st);
        return ISAC_OK;
      }
    }
    ISAC_PROF_COV0(st);
    hipLaunchKernelGGL((cov_mfma_small_kernel<NB>), dim3((unsigned)gx), dim3(256), 0, st, G, N, A, per, part);
    ISAC_HIP(hipGetLastError());
    ISAC_PROF_COV1(st);
    return ISAC_OK;
  });
}

// Ra of the context's NATIVE lazy echo grid (ctx->lazy: isac_mono_static_sensing_fused_dev with d_echo_grid == NULL) -- fft2D.m:106-107 without the array.
template <int QT>
static int launch_cov_lazy(isac_ctx* ctx, hipStream_t st, const LazyCovArgs& a, long long n_slabs, long long per, long long gx, double* part) {
  const size_t lds = sizeof(c64) * kCovLdsBufs * 4 * kCovSlabBlk;
  ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(cov_lazy_kernel<QT>), lds));
  ISAC_PROF_COV0(st);
  hipLaunchKernelGGL((cov_lazy_kernel<QT>), dim3((unsigned)gx), dim3(256), lds, st, a, n_slabs, per, part);
  ISAC_HIP(hipGetLastError());
  ISAC_PROF_COV1(st);
  return ISAC_OK;
}

// slabs of a lazy grid: 8 pair rows (k, k + 512) each, one 1024-subcarrier block pair after the other (CovLazyGenerator)
static long long lazy_slabs(int K, int L_whole, int* s_col_out) {
  int s_col = 0;
  for (int k0 = 0; k0 < K; k0 += 1024) s_col += (std::min(512, K - k0) + 7) / 8;
  *s_col_out = s_col;
  return (long long)L_whole * s_col;
}

bool isac_lazy_split_ok(long long T, int K, int L_whole) {
  int s_col = 0;
  const long long n_slabs = lazy_slabs(K, L_whole, &s_col);
  // (32-bit sample offsets below kCovOobOffset; the beam-sum's descriptor spans the whole waveform of up to 64 antennas -- the route's widest array -- and must end below it too)
  return T > 0 && T * 64 * (long long)sizeof(c64) < (1ll << 31) && n_slabs > 0 && n_slabs < (1ll << 31) - 4;
}

// Head of a CPI on the split route (ISAC_LAZY_COV_SPLIT, include/isac_lazy_cov.h): the noise term's workgroup partials into ctx->cov_noise, the beam-sums into ctx->beam.
int isac_cov_noise_beam_on(isac_ctx* ctx, hipStream_t st, const LazySplitFront& f) {
  if (!isac_lazy_split_ok(f.T, f.K, f.L_whole) || f.A <= 48 || f.A > 64 || f.Q < 1 || f.Q > 2) return fail(ctx, ISAC_ERR_UNSUPPORTED, "split lazy covariance: shape outside the route (49..64 antennas, one or two LoS targets)");
  // The main kernel walks the full slabs (noise_walk.hpp), the tail kernel the half slabs, packed; a shape without full slabs (K <= 512) still launches the main kernel,
  // for the beam-sum: its workgroups walk no slab, sum their units in the loop behind the slabs and leave zero partials.
  const NoiseWalk w = noise_walk(f.K);
  const long long n_slabs = (long long)f.L_whole * w.s_full, n_tail = (long long)f.L_whole * w.n_packed;
  long long gx, per, gt = 0, per_t = 0;
  if (n_slabs > 0) cov_staged_grid(n_slabs, gx, per);
  else { gx = std::max<long long>(1, std::min<long long>(bw_units(f.bw), 512)); per = 2; }
  if (n_tail > 0) noise_tail_grid(n_tail, gt, per_t);
  const int S = 32, n_tiles = CovPlan<4>::kTiles;
  ISAC_TRY(ensure(ctx, ctx->cov_noise, sizeof(double) * ((size_t)(gx + gt) + S) * n_tiles * 2 * 256));
  // The tail kernel depends on the seed and the shape alone: it goes to the second stream, behind everything the main stream holds so far (the last reader of cov_noise among
  // it) and beside everything from here on; covariance_lazy_split waits for it in front of the reduction.  ISAC_SINGLE_STREAM (fft2d.hip): in line, behind the main kernel.
  static const bool single_stream = std::getenv("ISAC_SINGLE_STREAM") != nullptr;
  hipStream_t st_tail = (single_stream || !ctx->stream2) ? st : ctx->stream2;
  if (gt > 0 && st_tail != st) {
    for (auto& e : ctx->ev_tail)
      if (!e) ISAC_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    ISAC_HIP(hipEventRecord(ctx->ev_tail[0], st));
    ISAC_HIP(hipStreamWaitEvent(st_tail, ctx->ev_tail[0], 0));
  }
  NoiseBeamArgs a{f.d_tx, f.steer_host ? nullptr : (const c64*)ctx->steer.p, (c64*)ctx->steer.p, (c64*)ctx->beam.p, f.T, f.seed, f.K, f.L_out, f.A, std::max(w.s_full, 1), f.bw};
  SteerArg sa{};
  if (f.steer_host) std::memcpy(sa.v, f.steer_host, sizeof(c64) * (size_t)f.A * f.Q);
  auto launch = [&](auto qc) -> int {
    constexpr int QT = decltype(qc)::value;
    const size_t lds = sizeof(c64) * (kCovLdsBufs * 4 * kCovSlabBlk + QT * kBeamSteerPitch) + sizeof(BeamUnitEntry) * kBeamStreamTab;
    ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(cov_noise_beam_kernel<QT>), lds));
    ISAC_PROF_COV0(st);
    hipLaunchKernelGGL((cov_noise_beam_kernel<QT>), dim3((unsigned)gx), dim3(256), lds, st, a, sa, n_slabs, per, (double*)ctx->cov_noise.p);
    ISAC_HIP(hipGetLastError());
    ISAC_PROF_COV1(st);
    return ISAC_OK;
  };
  ISAC_TRY(f.Q == 1 ? launch(std::integral_constant<int, 1>{}) : launch(std::integral_constant<int, 2>{}));
  ctx->split_tail_joined = true;
  if (gt > 0) {
    const NoiseTailArgs ta{f.seed, f.K, f.L_out, f.A, w};
    const size_t lds = sizeof(c64) * kCovLdsBufs * 4 * kCovSlabBlk;
    ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(cov_noise_tail_kernel), lds));
    hipLaunchKernelGGL(cov_noise_tail_kernel, dim3((unsigned)gt), dim3(256), lds, st_tail, ta, n_tail, per_t, (int)gx, (double*)ctx->cov_noise.p);
    ISAC_HIP(hipGetLastError());
    if (st_tail != st) {
      ISAC_HIP(hipEventRecord(ctx->ev_tail[1], st_tail));
      ctx->split_tail_joined = false;
    }
  }
  ctx->split_wg = (int)(gx + gt);
  return ISAC_OK;
}

// The tail of the split route, where cov_lazy_kernel runs on the other: reduce the noise partials to M / N, sum D's Gram matrix per symbol, assemble Ra.
static int covariance_lazy_split(isac_ctx* ctx, hipStream_t st, c64* Ra) {
  const LazyEcho& lz = ctx->lazy;
  const int S = 32, n_tiles = CovPlan<4>::kTiles, n_part = ctx->split_wg;
  const double inv_n = 1.0 / ((double)lz.K * (double)lz.L_out);
  double* part = (double*)ctx->cov_noise.p;
  double* part2 = part + (size_t)n_part * n_tiles * 2 * 256;
  c64* xc = (c64*)ctx->cov_xc.p;
  c64* H = xc + lazy_xc_elems(lz.L_whole, lz.A, lz.Q);
  c64* Mn = H + (size_t)lz.L_whole * lz.Q * lz.Q;
  if (!ctx->split_tail_joined) {                     // cov_noise_tail_kernel's partials (isac_cov_noise_beam_on)
    ISAC_HIP(hipStreamWaitEvent(st, ctx->ev_tail[1], 0));
    ctx->split_tail_joined = true;
  }
  hipLaunchKernelGGL(cov_reduce_slice_kernel, dim3(n_tiles, S), dim3(256), 0, st, (const double*)part, n_part, n_tiles, S, part2);
  ISAC_HIP(hipGetLastError());
  hipLaunchKernelGGL(cov_reduce_kernel, dim3(n_tiles), dim3(256, 4), 0, st, (const double*)part2, S, n_tiles, lz.A, inv_n, Mn);
  ISAC_HIP(hipGetLastError());
  const c64* srq = (const c64*)ctx->steer.p + (size_t)lz.A * lz.Q;
  auto tail = [&](auto qc) -> int {
    constexpr int QT = decltype(qc)::value;
    if constexpr (QT > 1) {                          // (one target: echo_range_xc_kernel has written xc)
      hipLaunchKernelGGL((cov_cross_kernel<QT>), dim3((unsigned)(lz.L_whole * lz.A)), dim3(256), 0, st, (const c64*)ctx->dgrid.p, lz.K, lz.L_whole, lz.L_out, lz.A, lz.seed, xc);
      ISAC_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL((cov_dgram_kernel<QT>), dim3((unsigned)lz.L_whole), dim3(256), 0, st, (const c64*)ctx->dgrid.p, lz.K, lz.L_whole, H);
    ISAC_HIP(hipGetLastError());
    hipLaunchKernelGGL((cov_assemble_kernel<QT>), dim3(1), dim3(256), 0, st, (const c64*)Mn, (const c64*)xc, (const c64*)H, srq, lz.A, lz.L_whole, lz.sig, inv_n, Ra);
    ISAC_HIP(hipGetLastError());
    return ISAC_OK;
  };
  ISAC_TRY(lz.Q == 1 ? tail(std::integral_constant<int, 1>{}) : tail(std::integral_constant<int, 2>{}));
  return ISAC_OK;
}

int isac_covariance_lazy_on(isac_ctx* ctx, hipStream_t st, isac_c64* d_Ra) {
  const LazyEcho& lz = ctx->lazy;
  if (!lz.valid || !lz.native || !d_Ra) return fail(ctx, ISAC_ERR_INVALID_ARG, "no native lazy echo grid on this context");
  if (lz.A <= 48 || lz.A > 64 || lz.Q < 1 || lz.Q > 2) return fail(ctx, ISAC_ERR_UNSUPPORTED, "lazy covariance: 49..64 antennas, one or two LoS targets");
  ctx->lazy_cov_used = lz.split ? ISAC_LAZY_COV_SPLIT : ISAC_LAZY_COV_REGENERATE;   // isac_ctx_get_lazy_cov_route_used
  if (lz.split) return covariance_lazy_split(ctx, st, (c64*)d_Ra);
  if ((long long)lz.K * lz.L_whole * 16 >= (1ll << 31)) return fail(ctx, ISAC_ERR_UNSUPPORTED, "lazy covariance: per-target grid of 2 GB or more");
  int s_col = 0;
  const long long n_slabs = lazy_slabs(lz.K, lz.L_whole, &s_col);
  if (n_slabs <= 0 || n_slabs >= (1ll << 31) - 4) return fail(ctx, ISAC_ERR_UNSUPPORTED, "lazy covariance: slab count out of range");
  long long gx, per;
  cov_staged_grid(n_slabs, gx, per);
  LazyCovArgs a{(const c64*)ctx->dgrid.p, (const c64*)ctx->steer.p + (size_t)lz.A * lz.Q, lz.sig, lz.seed, lz.K, lz.L_whole, lz.L_out, lz.A, s_col};
  return cov_partials_to_ra(ctx, st, (int)gx, CovPlan<4>::kTiles, lz.A, 1.0 / ((double)lz.K * (double)lz.L_out), (c64*)d_Ra, [&](double* part) -> int {
    return lz.Q == 1 ? launch_cov_lazy<1>(ctx, st, a, n_slabs, per, gx, part) : launch_cov_lazy<2>(ctx, st, a, n_slabs, per, gx, part);
  });
}

int isac_covariance_on(isac_ctx* ctx, hipStream_t st, const isac_c64* d_grid, int64_t N, int32_t A, isac_c64* d_Ra) {
  if (!d_grid || !d_Ra || N <= 0 || A <= 0) return fail(ctx, ISAC_ERR_INVALID_ARG, "bad arguments");
  const int nb = (A + 15) / 16;
  if (nb <= 4) {
    switch (nb) {
      case 1: return launch_cov_small<1>(ctx, st, (const c64*)d_grid, N, A, (c64*)d_Ra);
      case 2: return launch_cov_small<2>(ctx, st, (const c64*)d_grid, N, A, (c64*)d_Ra);
      case 3: return launch_cov_small<3>(ctx, st, (const c64*)d_grid, N, A, (c64*)d_Ra);
      default: return launch_cov_small<4>(ctx, st, (const c64*)d_grid, N, A, (c64*)d_Ra);
    }
  }
  {                                                  // 64 x 64 block pairs (any A > 64)
    const int n_blk = (A + 63) / 64;
    const int n_pairs = n_blk * (n_blk + 1) / 2;
    const long long total = (N + 15) / 16;
    long long n_chunks = 1024 / n_pairs;              // ~4 workgroups per CU over the launch, 2 resident
    if (n_chunks < 1) n_chunks = 1;
    if (n_chunks > total) n_chunks = total;
    if (N * 256 >= (1ll << 31)) return fail(ctx, ISAC_ERR_UNSUPPORTED, "covariance of more than 64 antennas: at most 2^23 - 1 samples per antenna");
    long long per = (total + n_chunks - 1) / n_chunks;
    per = (per + 1) & ~1ll;                           // the kernel walks slabs in pairs
    n_chunks = (total + per - 1) / per;
    ISAC_TRY(ensure(ctx, ctx->cov_part, sizeof(double) * (size_t)n_chunks * n_pairs * 16 * 2 * 256));
    ISAC_PROF_COV0(st);
    if (N * 512 < (1ll << 31)) {       // (32 antennas per staging descriptor: 32-bit offsets up to N x 31 x 16 B)
      const size_t lds = sizeof(c64) * kCovUImgs * kCovUImg;
      ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(cov_mfma_block_pl_kernel), (size_t)(lds)));
      hipLaunchKernelGGL(cov_mfma_block_pl_kernel, dim3((unsigned)(n_chunks * n_pairs)), dim3(256), lds, st, (const c64*)d_grid, (long long)N, A,
                         n_blk, n_pairs, 2 * per, (double*)ctx->cov_part.p);
    } else {
      const size_t lds = sizeof(c64) * 2 * kCovBufElems;
      ISAC_TRY(allow_lds(ctx, reinterpret_cast<const void*>(cov_mfma_block_kernel), (size_t)(lds)));
      hipLaunchKernelGGL(cov_mfma_block_kernel, dim3((unsigned)(n_chunks * n_pairs)), dim3(256), lds, st, (const c64*)d_grid, (long long)N, A,
                         n_blk, n_pairs, per, (double*)ctx->cov_part.p);
    }
    ISAC_HIP(hipGetLastError());
    ISAC_PROF_COV1(st);
    hipLaunchKernelGGL(cov_block_reduce_kernel, dim3(16, n_pairs), dim3(256, 4), 0, st, (const double*)ctx->cov_part.p, (int)n_chunks,
                       n_blk, n_pairs, A, 1.0 / (double)N, (c64*)d_Ra);
    ISAC_HIP(hipGetLastError());
    return ISAC_OK;
  }
}
