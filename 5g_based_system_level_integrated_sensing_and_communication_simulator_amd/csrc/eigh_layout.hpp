// The eigensolver's geometry, derived once (plain C++, no HIP: a host compiler builds and tests it -- tests/eigh_layout_host.cpp): the status record the kernels
// leave behind the eigenvalues, the carve of every kernel's dynamic LDS and the carve of ctx->eig_scratch.  Kernels form their pointers from these byte offsets,
// launchers request `bytes`; nothing else restates a size.  Offsets are bytes from the start of the dynamic LDS (of the scratch); complex regions and everything
// accessed as 16-byte quantities sit at multiples of 16.
#pragma once
#include <cstddef>

namespace isac {

constexpr int kTriWaves = 4;       // wavefronts of eigh_tridiag_small_kernel (eight: the same 124 us at n = 64 -- every step is a chain of LDS round trips, DPP sums and two barriers, ~5 000 cycles whatever the column count per wave)
constexpr int kBisectWaves = 4;    // eigenvalues per workgroup of eigh_bisect_kernel (one wavefront each)

// ---------------------------------------------------------------- the status record: ctx->eig_w [A] | EighInfo
// `status` negative = EighStatus; kEighReplayTimeout is recovered by isac_eigh_replay_recover once the stream is idle.  Cycle counters: clock64() >> 6 of one
// thread, printed under ISAC_DEBUG (doa.hip::eig_debug_print).  Words 1 and 2 and the tri_* words serve whichever kernel ran.
enum EighStatus : int {
  kEighRotStorage = -1,       // the QL recurrence ran out of rotation storage (no convergence)
  kEighReplayTimeout = -2,    // a live replay block gave up waiting for the recurrence
  kEighNotFinite = -3,        // the signal-subspace vectors are not finite (NaN / Inf in the covariance)
  kEighTridiagTimeout = -4,   // the distributed tridiagonalisation saw no progress for ~2 s
};
enum EighRoute : int { kEighRouteJacobi = -1, kEighRouteSubspace = -3 };   // markers in EighInfo::rotations
struct EighInfo {
  int status;         //  0  sweeps used (Jacobi, QL), 0 (subspace route), or an EighStatus
  int cyc_a;          //  1  Jacobi: rotation parameters | pipeline: the tridiagonalisation
  int cyc_b;          //  2  Jacobi: two-sided updates   | pipeline: formQ (zungtr)
  int cyc_ql;         //  3  the QL recurrence (Jacobi: 0)
  int cyc_replay;     //  4  the replay, block 0 (Jacobi: 0)
  int rotations;      //  5  plane rotations recorded by the QL recurrence, or an EighRoute
  int sticky;         //  6  kEighTridiagTimeout once the distributed tridiagonalisation timed out (the kernels behind it overwrite `status` and keep it), else 0
  int unused7;
  int sub_setup, sub_solve, sub_mgs, sub_back;   //  8..11  music_subspace_kernel: set-up, solves, Gram-Schmidt, back-transformation
  int tri_a;          // 12  small: reflector      | distributed: column + p published
  int tri_b;          // 13  small: matvec         | distributed: exchange wait
  int tri_c;          // 14  small: matvec + update | distributed: vector work
  int tri_d;          // 15                         | distributed: rank-2 update
};
static_assert(sizeof(EighInfo) == 64, "sixteen words behind the eigenvalues");
static_assert(offsetof(EighInfo, status) == 0 && offsetof(EighInfo, rotations) == 5 * 4 && offsetof(EighInfo, sticky) == 6 * 4, "status / route / sticky words");
static_assert(offsetof(EighInfo, sub_setup) == 8 * 4 && offsetof(EighInfo, tri_a) == 12 * 4, "counter words");

// ---------------------------------------------------------------- dynamic LDS, one carve per kernel
using LdsOff = int;                                        // a byte offset into (or a size of) a workgroup's LDS, at most 160 KB: 32 bits, as LDS addresses are (64-bit offsets cost the kernels 64-bit scalar shifts)
constexpr LdsOff kLdsC64 = 16, kLdsF64 = 8, kLdsI32 = 4;   // element sizes (isac::c64 = two doubles)
constexpr LdsOff kLdsTail = 64;                            // every request ends in 64 spare bytes

struct JacobiLds {   // jacobi_eigh_kernel, order A padded to the even n.  The first 128 bytes serve eigh_safe_scale before H is loaded.
  int n, h;
  LdsOff H, V;       // [n x n] c64 column-major each
  LdsOff rg;         // [h] c64: g_k
  LdsOff rc;         // [h] double: c_k
  LdsOff rp, rq;     // [h] int each: p_k, q_k
  LdsOff dirty;      // int: the sweep's convergence flag
  LdsOff end, bytes;
  static constexpr JacobiLds of(int A) {
    JacobiLds l{};
    l.n = (A + 1) & ~1; l.h = l.n / 2;
    const LdsOff n = l.n, h = l.h;
    l.H = 0; l.V = kLdsC64 * (n * n); l.rg = kLdsC64 * (2 * n * n);
    l.rc = l.rg + kLdsC64 * h; l.rp = l.rc + kLdsF64 * h; l.rq = l.rp + kLdsI32 * h; l.dirty = l.rq + kLdsI32 * h;
    l.end = l.dirty + kLdsI32; l.bytes = l.end + kLdsTail;
    return l;
  }
};

struct TridiagFusedLds {   // eigh_tridiag_fused_kernel
  LdsOff sv, sw, sn;       // [n] c64 each: pending reflector, pending w, the step's new reflector
  LdsOff spart;            // [4][n] c64: partial matrix-vector products
  LdsOff sred;             // [2 x 16] double: block reduction (and eigh_safe_scale)
  LdsOff end, bytes;
  static constexpr TridiagFusedLds of(int n_) {
    TridiagFusedLds l{};
    const LdsOff n = n_;
    l.sv = 0; l.sw = l.sv + kLdsC64 * n; l.sn = l.sw + kLdsC64 * n; l.spart = l.sn + kLdsC64 * n; l.sred = l.spart + kLdsC64 * (4 * n);
    l.end = l.sred + kLdsF64 * 32; l.bytes = l.end + kLdsTail;
    return l;
  }
};

struct TridiagSmallLds {   // eigh_tridiag_small_kernel (n <= 64)
  LdsOff M;                // [n x n] c64 column-major working matrix
  LdsOff spart;            // [kTriWaves][64] c64: partial matrix-vector products
  LdsOff svw;              // [kTriWaves][2][64] c64: each wave's own copy of v and w
  LdsOff sred;             // [32] double: eigh_safe_scale
  LdsOff end, bytes;
  static constexpr TridiagSmallLds of(int n_) {
    TridiagSmallLds l{};
    const LdsOff n = n_;
    l.M = 0; l.spart = kLdsC64 * (n * n); l.svw = l.spart + kLdsC64 * (kTriWaves * 64); l.sred = l.svw + kLdsC64 * (kTriWaves * 2 * 64);
    l.end = l.sred + kLdsF64 * 32; l.bytes = l.end + kLdsTail;
    return l;
  }
};

struct ReplayLds {     // eigh_replay_body: the replay kernels and the live replay blocks of eigh_formq_ql_kernel
  int bt;              // threads (= row items) per replay workgroup
  bool rows_in_lds;    // the workgroup's rows fit LDS (else they stream through global memory and only the rotations are staged)
  LdsOff rows;         // [n][bt] double (0 bytes when !rows_in_lds)
  LdsOff rows_bytes;
  LdsOff stage;        // [2][n] c64: the rotations of a sweep, double buffered
  LdsOff stage_bytes;
  LdsOff end, bytes;   // (no spare tail here)
  static constexpr ReplayLds of(int n_, int bt, bool rows_in_lds) {
    ReplayLds l{};
    const LdsOff n = n_;
    l.bt = bt; l.rows_in_lds = rows_in_lds;
    l.rows = 0; l.rows_bytes = rows_in_lds ? kLdsF64 * (bt * n) : 0;
    l.stage = l.rows_bytes; l.stage_bytes = kLdsC64 * (2 * n);
    l.end = l.bytes = l.stage + l.stage_bytes;
    return l;
  }
  // the launch geometry for order n: 64 rows per workgroup while they fit 150 KB, else 32; a thread stages at most 8 rotations per sweep (n <= 8 bt)
  static constexpr ReplayLds of(int n) {
    const int bt = (size_t)64 * n * kLdsF64 > 150 * 1024 ? 32 : 64;
    return of(n, bt, (size_t)bt * n * kLdsF64 <= 150 * 1024 && n <= 8 * bt);
  }
};

struct FormqQlLds {        // eigh_formq_ql_kernel: two views of the same bytes (block 0: zungtr, block 1: the QL wavefront); blocks >= 2: ReplayLds
  LdsOff sv, sp;           // zungtr: [n] c64 each -- the reflector, tau v^H Z
  LdsOff de, bde, rec;     // QL: [n] c64 each -- (d, e) interleaved, backup of the sweep window, rotations of the current sweep
  LdsOff unused;           // [4 n] double that no view uses: kept, the requested size decides which workgroups share a compute unit
  LdsOff end, bytes;
  LdsOff bytes_live;       // with live replay blocks in the launch: the larger of the two carves
  static constexpr FormqQlLds of(int n_) {
    FormqQlLds l{};
    const LdsOff n = n_;
    l.sv = l.de = 0; l.sp = l.bde = kLdsC64 * n; l.rec = l.bde + kLdsC64 * n; l.unused = l.rec + kLdsC64 * n;
    l.end = l.unused + kLdsF64 * (4 * n); l.bytes = l.end + kLdsTail;
    const LdsOff r = ReplayLds::of(n_).bytes;
    l.bytes_live = l.bytes > r ? l.bytes : r;
    return l;
  }
};

struct BisectLds {   // eigh_bisect_kernel
  LdsOff de;         // [n] c64: (.re = d_i, .im = e_{i-1}^2)
  LdsOff sred;       // [3][16] double
  LdsOff end, bytes;
  static constexpr BisectLds of(int n_) {
    BisectLds l{};
    l.de = 0; l.sred = kLdsC64 * n_;
    l.end = l.sred + kLdsF64 * 48; l.bytes = l.end + kLdsTail;
    return l;
  }
};

struct SubspaceLds {       // music_subspace_kernel: lane v owns column v of four [n][lv] planes
  int lmax;                // vectors the kernel can deliver for this order
  int lv;                  // row pitch of the planes (odd)
  LdsOff u0, u1, u2;       // [n][lv] double each: 1 / pivot, the two superdiagonals of U; afterwards [16][n] c64 at u0: a chunk of reflectors
  LdsOff y;                // [n][lv] double: right-hand sides / solutions = the vectors
  LdsOff sd, se;           // [n] double each
  LdsOff tau;              // [n] c64: reflector scalars
  LdsOff end, bytes;
  static constexpr SubspaceLds of(int n_, int lv_) {
    SubspaceLds l{};
    const LdsOff n = n_, plane = kLdsF64 * (n * lv_);
    l.lv = lv_;
    l.u0 = 0; l.u1 = l.u0 + plane; l.u2 = l.u1 + plane; l.y = l.u2 + plane; l.sd = l.y + plane; l.se = l.sd + kLdsF64 * n; l.tau = l.se + kLdsF64 * n;
    l.end = l.tau + kLdsC64 * n; l.bytes = l.end + kLdsTail;
    return l;
  }
  static constexpr SubspaceLds of(int n) {   // 120 KB of planes, at most 32 vectors; orders above 128: one vector per wavefront in the back-transformation (R = 4)
    int lmax = (int)(122880 / (32 * (size_t)n));
    lmax = lmax > 32 ? 32 : (lmax < 1 ? 1 : lmax);
    SubspaceLds l = of(n, lmax | 1);
    l.lmax = n > 128 && lmax > 16 ? 16 : lmax;
    return l;
  }
};

// ---------------------------------------------------------------- ctx->eig_scratch for order n (pointers: EighScratch, eigh_dev.hpp)
struct EighScratchLayout {
  // the exchange area of eigh_tridiag_dist_kernel -- per-wavefront (maximum, XCC id) | 2 parities x 256 rows x (p_i, next column's entry) as tagged granules -- at the
  // START of the scratch, wherever n puts the rest (the host zeroes a fresh allocation)
  static constexpr size_t kXchBytes = 2048 + 2 * 256 * 64;
  size_t xch;              // [kXchBytes], 128-byte aligned
  size_t M, Z;             // [n x n] c64 each
  size_t tau;              // [n] c64
  size_t rot;              // [rot_cap] c64
  size_t d, e;             // [n] double each
  size_t scale;            // [2] double (the first is used)
  size_t desc;             // [desc_cap][4] int, read as 8-byte words: 8-byte aligned (16 for even n)
  size_t cnt;              // [8] int
  size_t wsc;              // [n] double
  size_t end, bytes;
  long long rot_cap;
  int desc_cap;
  static constexpr EighScratchLayout of(int n_) {
    EighScratchLayout l{};
    const size_t n = (size_t)n_;
    l.rot_cap = (long long)16 * n_ * n_; l.desc_cap = 30 * n_ + 2;
    l.xch = 0; l.M = kXchBytes; l.Z = l.M + 16 * (n * n); l.tau = l.Z + 16 * (n * n); l.rot = l.tau + 16 * n;
    l.d = l.rot + 16 * (size_t)l.rot_cap; l.e = l.d + 8 * n; l.scale = l.e + 8 * (n + (n & 1));
    l.desc = l.scale + 8 * 2; l.cnt = l.desc + 4 * (4 * (size_t)l.desc_cap); l.wsc = l.cnt + 4 * 8;
    l.end = l.wsc + 8 * n;
    // the allocation, as it has been sized since the scratch has this carve: `end` + 272 spare bytes (264 for odd n).  The exchange tags depend on the first-use zeroing of exactly this size.
    l.bytes = 16 * ((size_t)2 * n * n + n + (size_t)16 * n * n) + 8 * (3 * n + 4) + 4 * (4 * (size_t)(30 * n + 2) + 8) + 256 + kXchBytes;
    return l;
  }
};

}  // namespace isac
