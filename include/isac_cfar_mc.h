/*
 * isac_cfar_mc.h -- the false-alarm and detection rates of the library's own CFAR detectors, measured by counting on the device: an ADDITIVE part of the C ABI of
 * libisac_hip.so under ISAC_ABI_VERSION 8 (one new entry point, no new struct, no new isac_abi_sizeof selector; nothing that isac.h, isac_targets.h or isac_cfar.h declare
 * changes).  Included by isac.h: include that.  Conventions: isac.h.
 *
 * The 'Auto' threshold factors of isac_cfar.h are roots of false-alarm equations solved on the host.  isac_cfar_monte_carlo draws noise, runs the per-CUT detector of
 * isac_cfar2d / isac_fft2d_redetect (the same device function) and counts: the sensing KPIs Pfa and Pd of the detector as built, CFAR loss included -- what the
 * fixed-threshold formula of sensing.detection.getPd (getPd.m:12, rocpfa) does not describe.  PROJECT-DEFINED.  A trial is a function of (seed, t)
 * only, t = 0 .. n_trials - 1: counts and flags do not depend on how the trials are spread over launches, workgroups or lanes, and a shorter run is a prefix of a longer one.
 *   generator       call j of trial t: Philox4x32-10 with key (seed lo, seed hi) and counter (t lo, t hi, 4, j) -- stream word 4 (0..3: the noise fields of isac.h) --
 *                   outputs o0..o3, w0 = o0 | o1 << 32, w1 = o2 | o3 << 32; the uniform of a word is u(w) = ((w >> 11) + 1) 2^-53, in (0, 1].
 *   training cells  N = n_train of them, unit-mean exponentials (the square-law noise of isac_cfar.h): T_{2j+1} = -ln u(w0), T_{2j+2} = -ln u(w1) of call j = 0 .. N/2 - 1.
 *   CUT             call j = N/2: E0 = -ln u(w0), theta = 2 pi (w1 >> 11) 2^-53.  With S_i = 10^(snr_db[i] / 10) (-inf: S_i = 0, the false-alarm point):
 *                     ISAC_TARGET_SW1  P_i = (1 + S_i) E0                                               (Swerling 1: exponential target power)
 *                     ISAC_TARGET_SW0  P_i = (sqrt(S_i) + sqrt(E0) cos theta)^2 + (sqrt(E0) sin theta)^2  (non-fluctuating target in complex Gaussian noise)
 *                   every SNR point of a trial sees the same training cells and the same CUT draw (common random numbers: n_det is non-decreasing in snr_db).
 *   detector        the per-CUT rule of isac_cfar.h on a 1 x (N + 1) window, guard 0: T_1 .. T_{N/2} in the N/2 columns before the CUT, the rest in the N/2 columns after it
 *                   (its "front half = the cells before the CUT"); alpha from m and pfa exactly as isac_cfar2d takes it ('Auto' from pfa, or 'Custom').
 *   result          flags[t + n_trials i] = 1 where P_i > alpha * noise estimate, else 0; n_det[i] = their sum over t.
 *   -ln u           evaluated in fp64 to a few ulp (not correctly rounded), cos / sin likewise: a (trial, SNR point) pair whose P_i lies within ~1e-14 relative of its
 *                   threshold may come out differently in another fp64 evaluation of the same rule.
 * Limits.  n_train even, 2 .. ISAC_CFAR_MC_MAX_TRAIN (odd or below 2: ISAC_ERR_INVALID_ARG -- every 2-D band gives an even N; more: ISAC_ERR_UNSUPPORTED); method, rank,
 * custom_factor and pfa as in isac_cfar2d; n_snr 1 .. 64; snr_db NaN or +inf: ISAC_ERR_INVALID_ARG; n_trials 1 .. 2^40; flags != NULL needs n_trials <= 2^22; an unknown
 * target_model: ISAC_ERR_INVALID_ARG.  Runs on the context's stream in launches of at most 2^28 trials and returns when complete.  Works in scratch of its own: the last
 * fft2D's state, every getter's answer, a pending submit and its result buffer stay untouched (as isac_fft2d_redetect).
 */
#ifndef ISAC_CFAR_MC_H
#define ISAC_CFAR_MC_H

#include "isac.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { ISAC_TARGET_SW0 = 0 /* non-fluctuating */, ISAC_TARGET_SW1 = 1 /* Swerling 1: exponential power */ };
#define ISAC_CFAR_MC_MAX_TRAIN 128
int isac_cfar_monte_carlo(isac_ctx* ctx, const isac_cfar_method* m, int32_t n_train, double pfa,
                          int32_t target_model, const double* snr_db, int32_t n_snr,
                          uint64_t n_trials, uint64_t seed,
                          uint64_t* n_det /* [n_snr] */, uint8_t* flags /* [n_trials x n_snr] column-major, or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* ISAC_CFAR_MC_H */
