/*
 * isac_subsample.h -- sub-sample range: fractional path delays in the multi-static echo and an off-grid range estimate: an ADDITIVE part of the C ABI of libisac_hip.so
 * under ISAC_ABI_VERSION 8 (two new entry points; no new struct, no new isac_abi_sizeof selector: flat arrays; nothing that include/isac.h or the other additive headers
 * declare changes).  STAND-ALONE: this header includes isac.h and is NOT included by it -- a host that wants these calls includes this file.  Conventions: isac.h.
 * PROJECT-DEFINED.
 *
 * ---- A. isac_multi_static_sensing_frac_dev: isac_multi_static_sensing_dev (isac_multistatic.h: its arguments in its order, its limits, its errors) with one more array behind
 * path_shift: path_frac [P], host, or NULL = all zero.  Path p is delayed by d_p + delta_p samples, d_p = path_shift[p], 0 <= delta_p = path_frac[p] < 1.  Once the coefficient
 * vectors of the integer delays are demodulated into D_p [n_sc x L] (the spectral synthesis of isac_multistatic.h),
 *     D_p[k, l]  <-  D_p[k, l] exp(-2 pi j (frac(fc delta_p / fs) + m_k delta_p / Nfft)),   m_k = k - n_sc / 2, k = 0 .. n_sc - 1 (the subcarrier's offset from DC)
 * -- the first term is what the carrier phase e^{j 2 pi fc (t - d - delta) Ts} of isac_multistatic.h gains, the second the delay of subcarrier m_k; the sum is reduced modulo
 * 1 before one sincos, fp64 throughout -- and the synthesis runs unchanged: echoGrid = sum_p a_p D_p + W.
 *   * path_frac NULL or every value exactly 0, in every noise mode: the bytes of isac_multi_static_sensing_dev, and not one launch more.  A path with delta_p == 0 beside
 *     others keeps its D_p untouched.
 *   * a non-zero delta_p is served in the spectral noise modes only (ISAC_NOISE_PHILOX_SPECTRAL, ISAC_NOISE_INJECTED_SPECTRAL); in NONE / INJECTED / PHILOX the call returns
 *     ISAC_ERR_UNSUPPORTED: the waveform route would need an interpolation filter.
 *   * a delta_p outside [0, 1) or not finite: ISAC_ERR_INVALID_ARG.  Like every check of that call, before any device work: a refused call launches and writes nothing.
 * VALIDITY.  The expression equals the physically delayed signal -- every OFDM symbol of the source, cyclic prefix included, evaluated at t - (d_p + delta_p) Ts -- while
 * d_p + delta_p <= CP / 2 - 1 samples (CP: the shorter cyclic prefix; the demodulator's window starts half a prefix into the symbol) and the source is a plain CP-OFDM
 * waveform (no inter-symbol windowing).  Beyond that it is the circular approximation that the integer part is already.  Not an error.  With a Doppler shift f the
 * demodulated symbol leaks between subcarriers, and a leaked term gets the ramp of the bin it lands on, not of the bin it left: against the physically delayed signal the
 * grid is then off by about sqrt(n_sc) 2 pi (f / SCS) delta / Nfft of its rms value (9e-3 of the largest value at 3 kHz, 60 kHz spacing, n_sc 132, Nfft 256) -- the size of the inter-carrier terms themselves.
 *
 * ---- B. isac_range_refine_dev: off-grid range of listed targets, from the two grids a caller of isac_fft2d_dev already has on the device.  For entry i: row_i, a 1-based rdm
 * row (e.g. a list's row[]), and nu_i, the Doppler frequency in cycles per symbol in the convention of isac_refine.h (natural symbol order; a grid column is
 * nu0 = (col - nFFT/2 - 1) / nFFT).  H = rx .* conj(tx) [K x L x A], w = kaiser(K, 3) (fft2D.m:40), rho the 0-based continuous extension of fft2D's range axis (row r is
 * IFFT bin r - 1):
 *     c_i[k, a] = sum_{l=0}^{L-1} H[k, l, a] e^{-2 pi j nu_i l}                        all L symbols, ascending
 *     Z_a(rho)  = nIFFT^{-1/2} sum_{k=0}^{K-1} w_k c_i[k, a] e^{+2 pi j k rho / nIFFT}
 *     P(rho)    = sum_a |Z_a(rho)|^2 / nFFT            x[a] = Z_a(rho) / sqrt(nFFT)
 *   1. probes     rho0 = row - 1, rho_g = rho0 + g / 8 for g = -8 .. 8 (17 probes over +-1 bin).
 *   2. peak       interior probes with P_g > P_{g-1} and P_g >= P_{g+1} are local maxima; the largest is taken, on a tie the lowest g.  None: status = 1, rho = rho0, power
 *                 and x at rho0.
 *   3. maximiser  rho* = the zero of P'(rho) = (2 / nFFT) sum_a Re(conj(Z_a) Z_a') in [rho_{g-1}, rho_{g+1}], by 40 halvings on the sign of P' (every entry the same
 *                 count; they leave 2.3e-13 bin of the bracket).  status = 0.
 *   4. outputs    rho = rho*, rng = rho* r_res, power = P(rho*), x at rho*.
 * probe_only != 0: steps 2-3 are skipped, status = 2, everything is evaluated at rho0.  At an integer row, x[a] times the library's range-axis weight of that row,
 * fftshift(kaiser(nIFFT, 3))[row - 1] (fft2D.m:45), is the snapshot isac_fft2d_refine_targets returns at the same nu: the kept rows carry that weight and this call
 * deliberately does not -- the weight belongs to a bin, not to a signal.
 * DETERMINISM.  Sums over l, over k and over a in fixed orders, no atomics: an entry's results are the same bits whatever its position in the input, whatever n, on every run.
 * SCRATCH.  The context's own, bounded by a chunk of 16 entries whatever n: 16 K A + 16 L + (A + 4) n complex values (the contracted planes of a chunk, its Doppler phasors,
 * the per-entry records).  The call reads each grid once per chunk of 16 entries, runs on the context's stream and returns when complete.  It needs no completed fft2D, and
 * leaves cached range rows, the lazy echo grid, every getter's answer and a pending submit untouched.  With isac_profile_enable(ctx, 1) the event pair of
 * isac_profile_last_kernel_ms brackets the Doppler contraction of the call's last chunk.
 *
 * ISAC_ERR_INVALID_ARG: a NULL grid (the lazy grid is not taken: isac_echo_grid_materialize_dev first); NULL ep; with n > 0 a NULL row, nu, status, rho, rng or power;
 * n < 0 or n > ISAC_MAX_TARGETS; K, L, A <= 0; K > ep->n_ifft; ep->n_fft <= 0; a row outside 1 .. n_ifft; a non-finite nu.  ISAC_ERR_CAPACITY: A > 256.
 * ISAC_ERR_UNSUPPORTED: K > 8192 (the phasors of one evaluation, K complex values, stay in LDS).  n == 0 returns ISAC_OK.  Everything is checked before any launch.
 *
 * OUT OF SCOPE: a MEX command; fractional delays in the time-domain noise modes, in isac_multi_static_channel_dev, isac_cancel_paths_dev and the fused and lazy mono-static
 * calls (the reference's ceil stays their model); a joint (rho, nu) iteration and a RELAX over range: two targets less than about two bins apart at ONE Doppler bias each
 * other (a NumPy experiment with tones 2.8 bins apart: 4e-3 bin at one Doppler, 1e-4 bin at different Dopplers); a direction rescan inside the call
 * (isac_resolve_directions takes the snapshots).
 */
#ifndef ISAC_SUBSAMPLE_H
#define ISAC_SUBSAMPLE_H

#include "isac.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISAC_RANGE_REFINE_CHUNK 16      /* entries per pass over the two grids */
#define ISAC_RANGE_REFINE_MAX_ANTS 256
#define ISAC_RANGE_REFINE_MAX_K 8192

int isac_multi_static_sensing_frac_dev(isac_ctx* ctx, const isac_c64* const* d_tx_waves /* [S] device pointers */, const int32_t* n_ants_src /* [S] */, int32_t n_sources,
                                       int64_t T, double fc, double fs, double n0, int32_t n_ants,
                                       int32_t n_paths, const int32_t* path_source, const int64_t* path_shift, const double* path_frac /* [P] in [0, 1), or NULL */,
                                       const double* path_doppler_hz, const double* path_gain,
                                       const isac_c64* path_tx_steering /* concatenated, path p: n_ants_src[path_source[p]] values */,
                                       const isac_c64* path_rx_steering /* [n_ants x n_paths] */,
                                       int noise_mode, const isac_c64* d_noise_unit, uint64_t seed,
                                       int32_t tx_dim_l, const isac_carrier* carrier, isac_c64* d_echo_grid /* [n_sc x max(L, tx_dim_l) x n_ants] */, int32_t* l_out);

int isac_range_refine_dev(isac_ctx* ctx, const isac_est_params* ep,
                          const isac_c64* d_rx_grid, const isac_c64* d_tx_grid /* [K x L x A] each, on the device */, int32_t K, int32_t L, int32_t A,
                          const int32_t* row /* 1-based rdm rows */, const double* nu /* cycles per symbol */, int32_t n, int32_t probe_only,
                          int32_t* status, double* rho, double* rng, double* power /* [n] each */, isac_c64* snapshots /* [A x n] or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* ISAC_SUBSAMPLE_H */
