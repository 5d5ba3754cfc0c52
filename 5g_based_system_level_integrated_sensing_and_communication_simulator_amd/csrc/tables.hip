// Cached device tables of libisac_hip (gfx950 only; host code): twiddles, the Box-Muller log table, the Kaiser and raised-cosine windows.  Each getter is its
// argument checks, its key in ctx->tables and the host code that makes the table on first use (cached_table, isac_internal.hpp).  The scan tables of direction
// finding are made the same way in doa.hip.
#include "isac_internal.hpp"

using namespace isac;

namespace {

// ---- host math mirrors of the MATLAB helpers the reference calls (product code, not the oracle)
double bessel_i0(double x) {  // power series, converges to < 1 ulp for |x| <= 10
  double q = 0.25 * x * x, term = 1.0, sum = 1.0;
  for (int k = 1; k < 200; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

std::vector<double> kaiser_window(int n, double beta) {  // Signal Processing Toolbox kaiser(n, beta); fft2D.m:135
  std::vector<double> w((size_t)n, 1.0);
  if (n == 1) return w;
  const int odd = n % 2;
  const double xind = (double)(n - 1) * (double)(n - 1);
  const int half = (n + 1) / 2;
  const double den = bessel_i0(std::fabs(beta));
  std::vector<double> h((size_t)half);
  for (int i = 0; i < half; ++i) {
    double xi = (double)i + 0.5 * (1 - odd);
    xi = 4.0 * xi * xi;
    h[(size_t)i] = std::fabs(bessel_i0(std::fabs(beta) * std::sqrt(1.0 - xi / xind)) / den);
  }
  // w = [h(half:-1:odd+1) h]
  int o = 0;
  for (int i = half - 1; i >= odd; --i) w[(size_t)o++] = h[(size_t)i];
  for (int i = 0; i < half; ++i) w[(size_t)o++] = h[(size_t)i];
  return w;
}

}  // namespace

// exp(-2 pi j m / n), m = 0..n-1
int isac_get_twiddles(isac_ctx* ctx, int n, const c64** out) {
  return cached_table(ctx, {kTwiddle, {n}}, out, [&](std::vector<c64>& w) {
    w.resize((size_t)n);
    for (int m = 0; m < n; ++m) {
      // exact octant reduction in long double, rounded once
      long double ang = -2.0L * 3.14159265358979323846264338327950288L * (long double)m / (long double)n;
      w[(size_t)m] = mk((double)cosl(ang), (double)sinl(ang));
    }
    // exact values on the axes
    w[0] = mk(1.0, 0.0);
    if (n % 4 == 0) { w[(size_t)n / 4] = mk(0.0, -1.0); w[(size_t)n / 2] = mk(-1.0, 0.0); w[(size_t)3 * n / 4] = mk(0.0, 1.0); }
  });
}

// {W512^0..511, W4096^0..7}: the LDS tables of Fft4096W in one contiguous run (bit-identical to entries 8 i / i of the 4096 table)
int isac_get_w512_pack(isac_ctx* ctx, const c64** out) {
  return cached_table(ctx, {kW512Pack}, out, [](std::vector<c64>& w) {
    w.resize(520);
    const long double two_pi = 2.0L * 3.14159265358979323846264338327950288L;
    for (int m = 0; m < 512; ++m) { const long double a = -two_pi * (long double)(8 * m) / 4096.0L; w[(size_t)m] = mk((double)cosl(a), (double)sinl(a)); }
    for (int m = 0; m < 8; ++m) { const long double a = -two_pi * (long double)m / 4096.0L; w[(size_t)512 + m] = mk((double)cosl(a), (double)sinl(a)); }
    w[0] = mk(1.0, 0.0); w[128] = mk(0.0, -1.0); w[256] = mk(-1.0, 0.0); w[384] = mk(0.0, 1.0); w[512] = mk(1.0, 0.0);
  });
}

// (1 / c_i, ln c_i) for the kLogTabSize mantissa buckets of the table-driven Box-Muller radius (echo_dev.hpp); c_i is
// the bucket centre in [0.5, 1); ln is taken of the reciprocal actually stored so that ln m = ln c_i + log1p(m / c_i - 1)
// holds to rounding.
int isac_get_logtab(isac_ctx* ctx, const c64** out) {
  return cached_table(ctx, {kLogTab}, out, [](std::vector<c64>& lt) {
    lt.resize(128);
    for (int i = 0; i < 128; ++i) {
      const long double c = 0.5L * (1.0L + ((long double)i + 0.5L) / 128.0L);
      const double inv = (double)(1.0L / c);
      lt[(size_t)i] = mk(inv, (double)(-logl((long double)inv)));
    }
  });
}

// rising raised-cosine edge of the OFDM symbol window (toolbox form, oracle/ofdm.py raised_cosine_edge)
int isac_get_rise_window(isac_ctx* ctx, int n_win, const double** out) {
  return cached_table(ctx, {kRiseWindow, {n_win}}, out, [&](std::vector<double>& w) {
    w.resize((size_t)n_win);
    for (int i = 1; i <= n_win; ++i) w[(size_t)i - 1] = 0.5 * (1.0 - std::sin(M_PI * (n_win + 1 - 2.0 * i) / (2.0 * n_win)));
  });
}

// kaiser(K, 3) over the subcarriers and fftshift(kaiser(n_ifft, 3)) over the range bins.  The subcarrier window is handed out as max(K, n_ifft) entries, +0.0 beyond K: it is
// the window of the zero-padded IFFT input (ifft(., nIFFT, 1), fft2D.m:43), so a kernel that indexes it with the unclamped input row (echo_range_sl_kernel, echo.hip) gets its
// zero padding from the product and needs no select; range_kernel and echo_range_kernel read it below K only.
int isac_get_windows(isac_ctx* ctx, int K, int n_ifft, const double** win_k, const double** win_r) {
  auto get = [&](int n, int n_pad, bool shifted, const double** out) {
    return cached_table(ctx, {shifted ? kKaiser3Shifted : kKaiser3, {n, n_pad}}, out, [&](std::vector<double>& w) {
      w = kaiser_window(n, 3.0);                                // fft2D.m:135 'kaiser', beta = 3
      if (shifted) {                                            // fftshift: out[i] = in[(i + ceil(n/2)) mod n]
        std::vector<double> s((size_t)n);
        const int sh = (n + 1) / 2;
        for (int i = 0; i < n; ++i) s[(size_t)i] = w[(size_t)((i + sh) % n)];
        w.swap(s);
      }
      if (n_pad > n) w.resize((size_t)n_pad, 0.0);
    });
  };
  ISAC_TRY(get(K, K > n_ifft ? K : n_ifft, false, win_k));
  ISAC_TRY(get(n_ifft, n_ifft, true, win_r));
  return ISAC_OK;
}
