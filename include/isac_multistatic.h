/*
 * isac_multistatic.h -- multi-static echo synthesis, paths from other cells' transmitters: an ADDITIVE part of the C ABI of libisac_hip.so under ISAC_ABI_VERSION 8 (two new
 * entry points; no new struct, no new isac_abi_sizeof selector: flat arrays; nothing that include/isac.h or the other additive headers declare changes).  Included by isac.h:
 * include that.  Conventions: isac.h.
 *
 * isac_basic_radar_channel_dev / isac_mono_static_sensing_dev hear the cell's own waveform, returned by its own targets (basicRadarChannel.m:39-64).  Here a PATH takes a
 * waveform from some source array, weights it with a transmit steering vector, delays it, Doppler-shifts it, scales it and spreads it over the receive array; a mono-static
 * target is the path "source = own array, both steering vectors equal".  The direct path from a neighbouring transmitter (inter-cell interference on sensing) and the
 * bistatic echo of a target another gNB illuminates are paths too.  PROJECT-DEFINED.
 *
 * Inputs: S source waveforms x_s [T x A_s] on the device (source 0 is by convention the cell's own; all sources share carrier, sample rate and slot timing: a synchronous
 * TDD network), a receive array of A = n_ants elements, and P paths (s_p, d_p >= 0 samples, f_p Hz, real gain g_p, tx steering b_p [A_{s_p}], rx steering a_p [A]).  Ts = 1 / fs:
 *     beam_p[u]  = sum_a x_{s_p}[u, a] b_p[a]                                                      antennas ascending, one complex fma each
 *     coef_p[t]  = g_p e^{j 2 pi f_p t Ts} e^{j 2 pi fc (t - d_p) Ts} beam_p[t - d_p] e^{-j 2 pi fc t Ts}     t >= d_p, else 0
 *     rx[t, r]   = sum_p coef_p[t] a_p[r]  +  sqrt(N0 / 2) noise[t, r] e^{-j 2 pi fc t Ts}                  isac_multi_static_channel_dev -> d_rx_wave [T x n_ants]
 *     echoGrid   = OFDM-demodulate(rx), padded to tx_dim_l symbols (monoStaticSensing.m:16-21)               isac_multi_static_sensing_dev -> d_echo_grid [n_sc x *l_out x n_ants]
 * -- the device expressions of the mono-static calls, with b_p in the beam-sum where they have a_q.  With S = 1, b_p = a_p, d_p = ceil(2 range / c / Ts), f_p = 2 v / lambda and
 * g_p = largeScaleFading of the LoS targets in their order, each call returns, bit for bit, what its mono-static counterpart returns, in every noise mode.
 *
 * Arrays.  d_tx_waves [S]: a HOST array of DEVICE pointers; n_ants_src [S]; path_source, path_shift, path_doppler_hz, path_gain [P]; path_tx_steering: the vectors b_p
 * concatenated in path order, path p holding n_ants_src[path_source[p]] values; path_rx_steering [n_ants x n_paths] column-major.  The path arrays and steering vectors are
 * host pointers, as in isac_radar_channel_params.
 *
 * Noise (isac_noise_mode).  isac_multi_static_channel_dev takes NONE / INJECTED / PHILOX; isac_multi_static_sensing_dev all five: the spectral modes demodulate the P
 * coefficient vectors and run the spectral synthesis of the mono-static call, echoGrid = sum_p a_p D_p + W.  The noise field is a function of the seed and the receive grid
 * only: the same seed gives the noise bits of the mono-static call.  d_noise_unit: [T x n_ants] (INJECTED) or [n_sc x *l_out x n_ants] (INJECTED_SPECTRAL).
 *
 * LIMITS: n_paths 1 .. 64; n_sources 1 .. 32; every A_s of a named source and n_ants 1 .. 256.  A path with shift >= T contributes nothing.  A source that no path names is
 * never read: its pointer may be NULL and its n_ants_src is not looked at.
 *
 * ISAC_ERR_NO_LOS: n_paths == 0 (the empty rxWaveform of basicRadarChannel.m:59,64).  ISAC_ERR_INVALID_ARG: a NULL argument (d_noise_unit only where the mode reads it; l_out
 * may be NULL); T, fs, n_sources, n_ants <= 0 or n_paths < 0; a path_source outside 0 .. n_sources - 1; a negative path_shift; a NULL waveform or an A_s <= 0 of a NAMED
 * source; a noise mode the call does not take.  ISAC_ERR_CAPACITY: more than 64 paths, more than 32 sources, more than 256 elements.  The carrier's errors and
 * ISAC_ERR_SHORT_WAVEFORM: isac_mono_static_sensing_dev's.  Everything is checked before any device work: a refused call launches nothing and writes nothing.
 * Like every echo call, both drop the context's cached range rows and lazy echo grid.  The result is an array that plain isac_fft2d_dev consumes with any transmit grid.
 *
 * OUT OF SCOPE: a MEX command; the fused range stage and the lazy echo grid (isac_mono_static_sensing_fused_dev stays mono-static); host-array variants; geometry (the Python
 * helper sensing.channelModels.multiStaticPaths turns node and target positions into paths); sources with different carriers, sample rates or slot timing.
 */
#ifndef ISAC_MULTISTATIC_H
#define ISAC_MULTISTATIC_H

#include "isac.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISAC_MULTISTATIC_MAX_PATHS 64
#define ISAC_MULTISTATIC_MAX_SOURCES 32
#define ISAC_MULTISTATIC_MAX_ANTS 256

int isac_multi_static_channel_dev(isac_ctx* ctx, const isac_c64* const* d_tx_waves /* [S] device pointers */, const int32_t* n_ants_src /* [S] */, int32_t n_sources,
                                  int64_t T, double fc, double fs, double n0, int32_t n_ants,
                                  int32_t n_paths, const int32_t* path_source, const int64_t* path_shift, const double* path_doppler_hz, const double* path_gain,
                                  const isac_c64* path_tx_steering /* concatenated, path p: n_ants_src[path_source[p]] values */,
                                  const isac_c64* path_rx_steering /* [n_ants x n_paths] */,
                                  int noise_mode, const isac_c64* d_noise_unit, uint64_t seed, isac_c64* d_rx_wave /* [T x n_ants] */);

int isac_multi_static_sensing_dev(isac_ctx* ctx, const isac_c64* const* d_tx_waves /* [S] device pointers */, const int32_t* n_ants_src /* [S] */, int32_t n_sources,
                                  int64_t T, double fc, double fs, double n0, int32_t n_ants,
                                  int32_t n_paths, const int32_t* path_source, const int64_t* path_shift, const double* path_doppler_hz, const double* path_gain,
                                  const isac_c64* path_tx_steering /* concatenated, path p: n_ants_src[path_source[p]] values */,
                                  const isac_c64* path_rx_steering /* [n_ants x n_paths] */,
                                  int noise_mode, const isac_c64* d_noise_unit, uint64_t seed,
                                  int32_t tx_dim_l, const isac_carrier* carrier, isac_c64* d_echo_grid /* [n_sc x max(L, tx_dim_l) x n_ants] */, int32_t* l_out);

#ifdef __cplusplus
}
#endif
#endif /* ISAC_MULTISTATIC_H */
