// The body of the straight-line fused synthesis + range kernels (echo.hip), included once per kernel: echo_range_sl_kernel<QT, NZ, STORE, GROUP> (XC = false) and
// echo_range_xc_kernel<QT> (XC = true) -- as text, not as a device function, so that every pointer stays the kernel's own argument (the instantiations of the first kernel
// are pinned instruction by instruction: tests/test_isa_cpu.py, tests/test_gpu_valu_diet.py; as a __forceinline__ device template taking the kernel's arguments the same text
// compiled to 1630 instead of 1622 instructions and 124 instead of 122 VGPRs in echo_range_sl_kernel<1, 1, false, 4>, and differently in all six instantiations).  The including kernel provides QT, NZ, STORE, GROUP, XC, its arguments, and xc.
// XC = true (the split lazy covariance, cov.hip): the column's cross term c_q[l, r] = sum_{k < K} w[k, l, r] conj(d_q[k, l]) of the unit noise with the target grids -- both
// already in registers here -- is summed beside the synthesis (per thread, then wave by wave in a fixed order) and stored at xc[(l A + r) QT + q].  Nothing else changes: the
// range rows keep their bits.
  static_assert(QT >= 1 && QT <= 2, "compile-time target count");
  static_assert(!XC || NZ == 1, "the cross term is of the Philox field");
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  c64* lds = reinterpret_cast<c64*>(smem_raw);
  using FFT = Fft4096W;
  constexpr int NT = FFT::NT, PER = FFT::PER, NG = PER / GROUP;
  const int tid = threadIdx.x;
  FFT fft;
  int l, r;
  if (!spectral_tile_map(blockIdx.x, L_whole, A, l, r)) return;       // padding workgroup of the tile grid (before any barrier)
  const long long colg = (long long)l + (long long)L_out * r;
  const c64* Dl = D + (long long)K * l;
  const long long d_stride = (long long)K * L_whole;
  const c64* ptx = txg + (long long)K * colg;
  const c64* nzc = NZ == 2 ? noise + (long long)K * colg : nullptr;
  const __amdgpu_buffer_rsrc_t rs_dst = buffer_of(grid + (long long)K * colg, (unsigned)K * (unsigned)sizeof(c64));
  c64 s[QT];
#pragma unroll
  for (int q = 0; q < QT; ++q) s[q] = steer_rq[(long long)r * QT + q];   // uniform: scalar registers
  struct Ld { c64 tx; double w; c64 d[QT]; c64 nz; };
  Ld ld[2][GROUP];
  auto load_group = [&](int g, int b) {
#pragma unroll
    for (int u = 0; u < GROUP; ++u) {
      const int k = tid + NT * (g * GROUP + u);
      const int kc = k < K ? k : K - 1;                                 // unconditional loads at a clamped row
      // every base below is uniform and the row's byte offset fits 32 bits (kc < 4096): as unsigned offsets the loads take the scalar-base + 32-bit vector-offset form --
      // one shift per element instead of a sign extension, a 64-bit shift and a 64-bit add per pointer
      const unsigned o16 = (unsigned)kc * (unsigned)sizeof(c64);
      auto at = [](const auto* base, unsigned off) { return *reinterpret_cast<decltype(base)>(reinterpret_cast<const char*>(base) + off); };
      Ld& e = ld[b][u];
      e.tx = at(ptx, o16);
      e.w = at(win_k, (unsigned)k * (unsigned)sizeof(double));          // the window of the zero-padded IFFT input: n_ifft entries, +0.0 from K on (isac_get_windows)
      if constexpr (NZ == 2) e.nz = at(nzc, o16);
#pragma unroll
      for (int q = 0; q < QT; ++q) e.d[q] = at(Dl + (long long)q * d_stride, o16);
    }
    asm volatile("" ::: "memory");                                      // (compiler-only) nothing of the next phase moves above these loads
  };
  fft.init_table(lds, tw, tid);                      // W512 (FFT twiddles); barrier inside
  load_group(0, 0);
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int j = 0; j < PER; ++j) fft.x[j] = mk(0.0, 0.0);               // unit noise first, then the range-IFFT input
  const int wave_k0 = __builtin_amdgcn_readfirstlane(tid & ~63);
  auto draw = [&](int c) {                                              // one Philox call: elements 2c, 2c + 1 (echo_dev.hpp pairing)
    if constexpr (NZ == 1) {
      const int j0 = 2 * c, j1 = j0 + 1;
      if (wave_k0 + NT * j0 < K) {                                      // (wavefront-uniform; VALU only inside)
        const uint64_t ctr = (uint64_t)(tid + NT * c) + (uint64_t)kSpectralSlotsPerColumn * (uint64_t)colg;
        uint32_t o[4];
        philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), kSpectralStream, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), o);
        fft.x[j0] = box_muller32_hw(o[0], o[1]);
        if (wave_k0 + NT * j1 < K) fft.x[j1] = box_muller32_hw(o[2], o[3]);
        if constexpr (XC) {                                             // rows from K on (a partial wave draws them) are not of the field: zero here, so that the cross term needs
          if (!(tid + NT * j0 < K)) fft.x[j0] = mk(0.0, 0.0);           // no mask of its own -- their range-IFFT input is a zero either way (e.w = +0.0 there)
          if (!(tid + NT * j1 < K)) fft.x[j1] = mk(0.0, 0.0);
        }
      }
    }
  };
  bool live = false;                                                    // any non-zero (or NaN) matched-filter sample in this column?
  auto consume = [&](int g, int b) {
    c64 xg[QT];                                                         // XC: this group's share of the cross term
#pragma unroll
    for (int q = 0; q < QT; ++q) xg[q] = mk(0.0, 0.0);
#pragma unroll
    for (int u = 0; u < GROUP; ++u) {
      const int j = g * GROUP + u, k = tid + NT * j;
      const Ld& e = ld[b][u];
      if constexpr (XC) {
#pragma unroll
        for (int q = 0; q < QT; ++q) {
          xg[q] = fma(fft.x[j], conj(e.d[q]), xg[q]);
          asm volatile("" : "+v"(xg[q].re), "+v"(xg[q].im));              // (compiler-only: the sum is complete HERE, element by element, like the value above)
        }
      }
      const c64 v = spectral_echo_value<QT, NZ != 0>(e.d, s, NZ == 2 ? e.nz : fft.x[j], sig);
      if constexpr (STORE) buffer_store_c64_nt(rs_dst, (unsigned)k * (unsigned)sizeof(c64), v);   // echoGrid(k, l, r); k >= K: dropped by the bounds check
      else asm volatile("" ::"v"(v.re), "v"(v.im) : "memory");          // (compiler-only: the element is complete HERE, as in the storing form -- without this anchor the scheduler
                                                                        //  interleaves the eight elements and the two-target form spills 35 registers)
      const c64 y = mul_conj(v, e.tx) * e.w;                            // fft2D.m:37,:43 (same order as range_kernel); k >= K: e.w = +0.0, so y is a signed zero --
      live |= (y.re != 0.0) | (y.im != 0.0);                            // ifft(., nIFFT, 1) zero-pads at the end -- without a select per element (v, e.tx come from row K - 1:
      fft.x[j] = y;                                                     // finite wherever that row's own product is)
    }
    // The group sums wait in the transform's data image, which is idle until the range IFFT (slot (g, q, tid): thread-private, no barrier), not in registers held across
    // the whole column.
    if constexpr (XC) {
#pragma unroll
      for (int q = 0; q < QT; ++q) lds[(g * QT + q) * NT + tid] = xg[q];
    }
  };
#pragma unroll
  for (int g = 0; g < NG; ++g) {
#pragma unroll
    for (int c = g * GROUP / 2; c < (g + 1) * GROUP / 2; ++c) draw(c);
    __builtin_amdgcn_sched_barrier(0);
    if (g + 1 < NG) load_group(g + 1, (g + 1) & 1);
    consume(g, g & 1);
    __builtin_amdgcn_sched_barrier(0);
  }
  c64* yd = ymid + (long long)n_rows * colg;
  c64* xs = lds + FFT::LDS_ELEMS;                                       // XC: one partial per wave and target, behind the transform's own LDS
  if constexpr (XC) {
    static_assert(NG * QT * NT <= FFT::IMG, "the group sums fit the data image");
    c64 xacc[QT];
#pragma unroll
    for (int q = 0; q < QT; ++q) {
      xacc[q] = lds[q * NT + tid];
#pragma unroll
      for (int g = 1; g < NG; ++g) xacc[q] += lds[(g * QT + q) * NT + tid];
#pragma unroll
      for (int m = 32; m > 0; m >>= 1) { xacc[q].re += __shfl_xor(xacc[q].re, m); xacc[q].im += __shfl_xor(xacc[q].im, m); }
      if ((tid & 63) == 0) xs[(tid >> 6) * QT + q] = xacc[q];
    }
  }
  const bool any_live = __syncthreads_or(live);
  if constexpr (XC) {
    if (tid < QT) {
      c64 sum = xs[tid];
      for (int w = 1; w < NT / 64; ++w) sum += xs[w * QT + tid];
      xc[((long long)l * A + r) * QT + tid] = sum;
    }
  }
  if (!any_live) {                                                      // zero-filled 'S' slot column (see echo_range_kernel)
    for (int rr = tid; rr < n_rows; rr += NT) yd[rr] = mk(0.0, 0.0);
    return;
  }
  fft.init_twiddles_lds(lds, tid);
  const int blk = FFT::block_of_rows(row_lo, n_rows);
  fft.template transform<+1>(lds, tw, tid, blk);
  auto put = [&](int n, c64 v) {
    const int rr = n - row_lo;
    const double wr = win_r[n];
    if (rr >= 0 && rr < n_rows) yd[rr] = ((v * inv_n) * sqrt_n) * wr;            // fft2D.m:44-45
  };
  if (blk >= 0) fft.drain_block(put, tid, blk);
  else fft.drain(put, tid);
