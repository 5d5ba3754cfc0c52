// Stand-alone check of csrc/eigh_layout.hpp (no HIP, no library): the status record, every kernel's LDS carve and the carve of the eigensolver's scratch, for every
// order the dispatch rules of eigh.hip / music.hip / doa.hip send to each kernel.  Per carve: the regions are in order and do not overlap, every offset is aligned to
// its element (16 bytes for complex data and for what is accessed as 16-byte quantities), the last region ends at `end` <= `bytes`, `bytes` fits the 160 KB a
// workgroup can have, and `bytes` equals the size the launchers requested before the carves had a header -- those formulas are written out below as they stood.
// Built and run by tests/test_eigh_layout_cpu.py; exit status 0 = every check held.
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <initializer_list>

#include "eigh_layout.hpp"

namespace {

using namespace isac;
struct c64 { double re, im; };                            // as isac::c64 (isac_common.hpp)
constexpr size_t kLdsMax = 160 * 1024;

int failures = 0;
long long checks = 0;

void eq(const char* what, int n, long long got, long long want) {
  ++checks;
  if (got != want) { std::fprintf(stderr, "%s, n = %d: %lld, expected %lld\n", what, n, got, want); ++failures; }
}
void ok(const char* what, int n, bool cond) {
  ++checks;
  if (!cond) { std::fprintf(stderr, "%s, n = %d: does not hold\n", what, n); ++failures; }
}

struct Region { const char* name; long long off, size, align; };
// regions in carve order: aligned, no overlap, the last one ends at `end`, end <= bytes <= limit
void carve(const char* kernel, int n, std::initializer_list<Region> regions, long long end, long long bytes, long long limit) {
  long long at = 0;
  for (const Region& r : regions) {
    ++checks;
    if (r.off < at || r.off % r.align != 0 || r.size < 0) {
      std::fprintf(stderr, "%s, n = %d: region %s at %lld (size %lld, alignment %lld) after %lld\n", kernel, n, r.name, r.off, r.size, r.align, at);
      ++failures;
    }
    at = r.off + r.size;
  }
  eq(kernel, n, end, at);
  ok(kernel, n, end <= bytes && bytes <= limit);
}

}  // namespace

int main() {
  // ---- the status record
  eq("sizeof(EighInfo)", 0, sizeof(EighInfo), 64);
  eq("offsetof status", 0, offsetof(EighInfo, status), 0);
  eq("offsetof cyc_a", 0, offsetof(EighInfo, cyc_a), 1 * 4);
  eq("offsetof cyc_b", 0, offsetof(EighInfo, cyc_b), 2 * 4);
  eq("offsetof cyc_ql", 0, offsetof(EighInfo, cyc_ql), 3 * 4);
  eq("offsetof cyc_replay", 0, offsetof(EighInfo, cyc_replay), 4 * 4);
  eq("offsetof rotations", 0, offsetof(EighInfo, rotations), 5 * 4);
  eq("offsetof sticky", 0, offsetof(EighInfo, sticky), 6 * 4);
  eq("offsetof sub_setup", 0, offsetof(EighInfo, sub_setup), 8 * 4);
  eq("offsetof sub_solve", 0, offsetof(EighInfo, sub_solve), 9 * 4);
  eq("offsetof sub_mgs", 0, offsetof(EighInfo, sub_mgs), 10 * 4);
  eq("offsetof sub_back", 0, offsetof(EighInfo, sub_back), 11 * 4);
  eq("offsetof tri_a", 0, offsetof(EighInfo, tri_a), 12 * 4);
  eq("offsetof tri_b", 0, offsetof(EighInfo, tri_b), 13 * 4);
  eq("offsetof tri_c", 0, offsetof(EighInfo, tri_c), 14 * 4);
  eq("offsetof tri_d", 0, offsetof(EighInfo, tri_d), 15 * 4);
  eq("status codes", 0, kEighRotStorage * 1000 + kEighReplayTimeout * 100 + kEighNotFinite * 10 + kEighTridiagTimeout, -1234);
  eq("route markers", 0, kEighRouteJacobi * 10 + kEighRouteSubspace, -13);

  // ---- jacobi_eigh_kernel: isac_eigh_dev, A = 1..16
  for (int A = 1; A <= 16; ++A) {
    const JacobiLds l = JacobiLds::of(A);
    const int n = (A + 1) & ~1;
    eq("Jacobi n", A, l.n, n); eq("Jacobi h", A, l.h, n / 2);
    const long long nn = (long long)n * n, h = n / 2;
    carve("Jacobi", A, {{"H", l.H, 16 * nn, 16}, {"V", l.V, 16 * nn, 16}, {"rg", l.rg, 16 * h, 16}, {"rc", l.rc, 8 * h, 8}, {"rp", l.rp, 4 * h, 4},
                        {"rq", l.rq, 4 * h, 4}, {"dirty", l.dirty, 4, 4}}, l.end, l.bytes, kLdsMax);
    ok("Jacobi: 16 doubles for eigh_safe_scale", A, l.bytes >= 128);
    eq("Jacobi bytes", A, l.bytes, sizeof(c64) * ((size_t)2 * n * n + n / 2) + sizeof(double) * (n / 2) + sizeof(int) * (n + 1) + 64);
  }
  // ---- eigh_tridiag_small_kernel: isac_eigh_top (3..16) and isac_eigh_dev (17..64)
  for (int n = 3; n <= 64; ++n) {
    const TridiagSmallLds l = TridiagSmallLds::of(n);
    carve("small tridiag", n, {{"M", l.M, 16LL * n * n, 16}, {"spart", l.spart, 16LL * kTriWaves * 64, 16}, {"svw", l.svw, 16LL * kTriWaves * 2 * 64, 16},
                               {"sred", l.sred, 8 * 32, 8}}, l.end, l.bytes, 112 * 1024);   // (the launcher allows this kernel 112 KB)
    eq("small tridiag bytes", n, l.bytes, sizeof(c64) * ((size_t)n * n + kTriWaves * 64 + kTriWaves * 2 * 64) + sizeof(double) * 32 + 64);
  }
  // ---- eigh_tridiag_fused_kernel: 65..1024 (all of them with ISAC_EIG_TRIDIAG_DIST=0, else beyond 256)
  for (int n = 65; n <= 1024; ++n) {
    const TridiagFusedLds l = TridiagFusedLds::of(n);
    carve("fused tridiag", n, {{"sv", l.sv, 16LL * n, 16}, {"sw", l.sw, 16LL * n, 16}, {"sn", l.sn, 16LL * n, 16}, {"spart", l.spart, 64LL * n, 16},
                               {"sred", l.sred, 8 * 32, 8}}, l.end, l.bytes, kLdsMax);
    eq("fused tridiag bytes", n, l.bytes, sizeof(c64) * 7 * (size_t)n + sizeof(double) * 32 + 64);
  }
  // ---- eigh_replay_body and eigh_formq_ql_kernel: 17..1024
  int n_live = 0;
  for (int n = 17; n <= 1024; ++n) {
    // the launch geometry as isac_eigh_ql_dev / launch_replay_offline derived it
    const int bt = (size_t)64 * n * sizeof(double) > 150 * 1024 ? 32 : 64;
    const size_t rows3 = (size_t)bt * n * sizeof(double), stage3 = sizeof(c64) * 2 * (size_t)n;
    const bool lds_replay = rows3 <= 150 * 1024 && n <= 8 * bt;
    const ReplayLds g = ReplayLds::of(n);
    eq("replay bt", n, g.bt, bt); eq("replay rows fit LDS", n, g.rows_in_lds, lds_replay);
    if (lds_replay) { eq("replay rows bytes", n, g.rows_bytes, (long long)rows3); eq("replay bytes", n, g.bytes, (long long)(rows3 + stage3)); ++n_live; }
    eq("replay stage bytes", n, g.stage_bytes, (long long)stage3);
    for (int b : {32, 64}) {                               // both row counts, wherever that many rows fit
      if ((size_t)b * n * sizeof(double) > 150 * 1024 || n > 8 * b) continue;
      const ReplayLds l = ReplayLds::of(n, b, true);
      carve("replay (rows in LDS)", n, {{"rows", l.rows, 8LL * b * n, 8}, {"stage", l.stage, 32LL * n, 16}}, l.end, l.bytes, kLdsMax);
      eq("replay (rows in LDS) bytes", n, l.bytes, (long long)((size_t)b * n * sizeof(double) + stage3));
    }
    const ReplayLds s = ReplayLds::of(n, 256, false);      // the streaming kernel: 256 threads, rotations only
    carve("replay (streaming)", n, {{"stage", s.stage, 32LL * n, 16}}, s.end, s.bytes, 64 * 1024);   // (no allow_lds call: the default limit)
    eq("replay (streaming) bytes", n, s.bytes, (long long)stage3);

    const FormqQlLds q = FormqQlLds::of(n);
    carve("formQ/QL, zungtr view", n, {{"sv", q.sv, 16LL * n, 16}, {"sp", q.sp, 16LL * n, 16}, {"(unused by this view)", q.rec, 16LL * n, 16},
                                       {"unused", q.unused, 32LL * n, 8}}, q.end, q.bytes, kLdsMax);
    carve("formQ/QL, QL view", n, {{"de", q.de, 16LL * n, 16}, {"bde", q.bde, 16LL * n, 16}, {"rec", q.rec, 16LL * n, 16}, {"unused", q.unused, 32LL * n, 8}},
          q.end, q.bytes, kLdsMax);
    const size_t lds2 = sizeof(c64) * 3 * (size_t)n + sizeof(double) * 4 * (size_t)n + 64;
    eq("formQ/QL bytes", n, q.bytes, (long long)lds2);
    if (lds_replay) {
      eq("formQ/QL bytes with live replay blocks", n, q.bytes_live, (long long)std::max(lds2, rows3 + stage3));
      ok("formQ/QL live bytes fit", n, (size_t)q.bytes_live <= kLdsMax);
    }
  }
  ok("orders with a live replay", 0, n_live == 300 - 17 + 1);   // 64 n doubles <= 150 KB: n <= 300
  // ---- eigh_bisect_kernel and music_subspace_kernel: 3..256 (isac_music_subspace_ok)
  for (int n = 3; n <= 256; ++n) {
    const BisectLds b = BisectLds::of(n);
    carve("bisect", n, {{"de", b.de, 16LL * n, 16}, {"sred", b.sred, 8 * 48, 8}}, b.end, b.bytes, 64 * 1024);
    eq("bisect bytes", n, b.bytes, sizeof(c64) * (size_t)n + sizeof(double) * 48 + 64);

    int lmax = (int)(122880 / (32 * (size_t)n));
    lmax = lmax > 32 ? 32 : (lmax < 1 ? 1 : lmax);
    const int lv = lmax | 1;                           // odd pitch
    if (n > 128 && lmax > 16) lmax = 16;               // one vector per wavefront in the back-transformation of the R = 4 instantiation
    const SubspaceLds l = SubspaceLds::of(n);
    eq("subspace lmax", n, l.lmax, lmax); eq("subspace lv", n, l.lv, lv);
    const long long plane = 8LL * n * lv;
    carve("subspace", n, {{"u0", l.u0, plane, 16}, {"u1", l.u1, plane, 8}, {"u2", l.u2, plane, 8}, {"y", l.y, plane, 8}, {"sd", l.sd, 8LL * n, 8},
                          {"se", l.se, 8LL * n, 8}, {"tau", l.tau, 16LL * n, 16}}, l.end, l.bytes, 150 * 1024);   // (the launcher allows this kernel 150 KB)
    ok("subspace: a chunk of 16 reflectors fits the three elimination planes", n, 16LL * 16 * n <= 3 * plane);
    ok("subspace: a lane per vector", n, l.lmax <= l.lv && l.lmax <= 64);
    eq("subspace bytes", n, l.bytes, sizeof(double) * ((size_t)4 * n * lv + 4 * (size_t)n) + 64);
    const SubspaceLds k = SubspaceLds::of(n, lv);      // the kernel's call
    ok("subspace: kernel and launcher agree", n, k.u1 == l.u1 && k.u2 == l.u2 && k.y == l.y && k.sd == l.sd && k.se == l.se && k.tau == l.tau && k.bytes == l.bytes);
  }
  // ---- ctx->eig_scratch: 1..1024
  for (int n = 1; n <= 1024; ++n) {
    const EighScratchLayout l = EighScratchLayout::of(n);
    const long long nn = (long long)n * n;
    eq("scratch rot_cap", n, l.rot_cap, 16 * nn); eq("scratch desc_cap", n, l.desc_cap, 30 * n + 2);
    // desc is read as 8-byte words and wsc as doubles: 8 bytes is what they need; 16 is what they get for even n only (n + (n & 1) + 2 doubles behind d [n], which is
    // 16-byte aligned: an odd count for odd n)
    const long long a16 = n % 2 == 0 ? 16 : 8;
    carve("scratch", n, {{"xch", (long long)l.xch, (long long)EighScratchLayout::kXchBytes, 128}, {"M", (long long)l.M, 16 * nn, 16}, {"Z", (long long)l.Z, 16 * nn, 16},
                         {"tau", (long long)l.tau, 16LL * n, 16}, {"rot", (long long)l.rot, 16 * l.rot_cap, 16}, {"d", (long long)l.d, 8LL * n, 16},
                         {"e", (long long)l.e, 8LL * n, 8}, {"scale", (long long)l.scale, 8 * 2, 8}, {"desc", (long long)l.desc, 16LL * l.desc_cap, a16},
                         {"cnt", (long long)l.cnt, 4 * 8, 4}, {"wsc", (long long)l.wsc, 8LL * n, a16}}, (long long)l.end, (long long)l.bytes, 1LL << 40);
    eq("scratch: the exchange area comes first", n, (long long)l.xch, 0);
    eq("scratch bytes", n, (long long)l.bytes,
       (long long)(sizeof(c64) * ((size_t)2 * n * n + n + (size_t)16 * n * n) + sizeof(double) * (3 * n + 4) + sizeof(int) * (4 * (size_t)(30 * n + 2) + 8) + 256 +
                   (2048 + 2 * 256 * 64)));
    eq("scratch spare bytes", n, (long long)(l.bytes - l.end), n % 2 == 0 ? 272 : 264);
  }
  if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  std::printf("eigh_layout: %lld checks OK\n", checks);
  return 0;
}
