/*
 * isac_cancel_paths.h -- reference-signal cancellation on the received waveform (the "extensive cancellation algorithm", ECA, of passive and multi-static radar): an ADDITIVE
 * part of the C ABI of libisac_hip.so under ISAC_ABI_VERSION 8 (one new entry point; no new struct, no new enum value, no new isac_abi_sizeof selector: flat arrays; nothing
 * that include/isac.h or the other additive headers declare changes).  Included by isac.h: include that.  Conventions: isac.h.
 *
 * A neighbour's direct path raises the floor of every range-Doppler map formed with the cell's own grid (include/isac_multistatic.h): its data does not compress.  In a
 * system-level simulator the neighbour's waveform and the geometry are known, so the interfering signals can be projected out of the received waveform before OFDM
 * demodulation -- on the waveform, not per subcarrier: a delay beyond the cyclic prefix arrives as inter-symbol and inter-carrier terms that no per-subcarrier fit sees,
 * while a delayed reference matches a whole-sample channel delay exactly.  PROJECT-DEFINED.
 *
 * Inputs: the received waveform Y [T x A] on the device (A = n_ants), the S source waveforms of isac_multi_static_channel_dev, and M references, each described like a path of
 * isac_multistatic.h without gain and without receive steering: source s_m, shift d_m >= 0 samples, Doppler f_m Hz, transmit steering b_m [A_{s_m}].  The fit finds one complex
 * coefficient per reference and receive element.
 *     r_m[t]  = coef_m[t] of isac_multistatic.h with g = 1 (the delayed, Doppler-shifted beam-sum with the channel's carrier phases; 0 for t < d_m)      R = [r_0 .. r_{M-1}]  [T x M]
 *     G       = R^H R                      [M x M]     then G_mm <- G_mm (1 + loading), loading >= 0
 *     B       = R^H Y                      [M x A]
 *     C       = G^-1 B                     Cholesky, references in input order                                                  -> coef [M x A] column-major
 *     Y'      = Y - R C                    [T x A]                                                                              -> d_out
 *     power_in[a] = sum_t |Y[t, a]|^2,  power_out[a] = sum_t |Y'[t, a]|^2 (summed from the values written)                      -> power: power_in [A], then power_out [A]
 * Every sum over t is a fixed-order reduction of per-workgroup partials (no atomics): the same call gives the same bits every time, in place or out of place.
 *
 * DEPENDENT REFERENCES.  Reference m is dependent when G_mm == 0 (an all-zero column, e.g. d_m >= T) or when its Cholesky pivot is <= 1e-10 G_mm (the loaded diagonal): the
 * part of r_m orthogonal to the earlier references holds no more than 1e-10 of its energy.  The call then returns ISAC_ERR_INVALID_ARG, writes the FIRST such m to *dependent
 * and leaves d_out untouched (in place: Y keeps its bits) -- the test runs on the device and the subtraction reads its flag; coef and power are not written.  On success
 * *dependent = -1.
 *
 * Arrays.  d_tx_waves [S]: a HOST array of DEVICE pointers; n_ants_src [S]; ref_source, ref_shift, ref_doppler_hz [M]; ref_tx_steering: the vectors b_m concatenated in
 * reference order, reference m holding n_ants_src[ref_source[m]] values -- host pointers, as in isac_multi_static_channel_dev.  d_out may be d_rx_wave (in place) or a buffer
 * that does not overlap it.  coef (host, [M x A] column-major), power (host, 2 A doubles: power_in [A], then power_out [A]) and dependent (host) may each be NULL.
 *
 * LIMITS: n_refs 1 .. 32; n_sources 1 .. 32; every A_s of a named source and n_ants 1 .. 256.  A source that no reference names is never read: its pointer may be NULL.
 *
 * ISAC_ERR_INVALID_ARG: a NULL argument (but coef, power, dependent); T, fs, n_sources, n_ants or n_refs <= 0; a ref_source outside 0 .. n_sources - 1; a negative ref_shift;
 * a NULL waveform or an A_s <= 0 of a NAMED source; a negative or non-finite loading; d_out partially overlapping d_rx_wave; a dependent reference (above).
 * ISAC_ERR_CAPACITY: more than 32 references, more than 32 sources, more than 256 elements.  Everything but the dependence test is checked before any device work: such a
 * refused call launches nothing and writes nothing, *dependent included.
 * The call returns after its status record has been read back: one device -> host copy behind the last kernel; the solve stays on the device and no host round trip sits between
 * the passes.  The reference columns are formed by the multi-static calls' own coefficient kernel in their scratch, so this is an echo call: like every echo call, it drops the
 * context's cached range rows and lazy echo grid.
 *
 * OUT OF SCOPE: a MEX command; cancellation inside the fused or lazy mono-static calls or with spectral-domain noise (the waveform never exists there); estimating unknown
 * delays (the Python helper sensing.channelModels.referencePaths expands a known delay into neighbouring taps).
 */
#ifndef ISAC_CANCEL_PATHS_H
#define ISAC_CANCEL_PATHS_H

#include "isac.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISAC_CANCEL_PATHS_MAX_REFS 32

int isac_cancel_paths_dev(isac_ctx* ctx, const isac_c64* const* d_tx_waves /* [S] device pointers */, const int32_t* n_ants_src /* [S] */, int32_t n_sources,
                          int64_t T, double fc, double fs, int32_t n_ants,
                          int32_t n_refs, const int32_t* ref_source, const int64_t* ref_shift, const double* ref_doppler_hz,
                          const isac_c64* ref_tx_steering /* concatenated, reference m: n_ants_src[ref_source[m]] values */,
                          double loading, const isac_c64* d_rx_wave /* [T x n_ants] */, isac_c64* d_out /* [T x n_ants]; may be d_rx_wave */,
                          isac_c64* coef /* host [n_refs x n_ants] or NULL */, double* power /* host, power_in [n_ants] then power_out [n_ants], or NULL */, int32_t* dependent /* host or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* ISAC_CANCEL_PATHS_H */
