/*
 * isac_beams.h -- beamformed detection on the last fft2D: an ADDITIVE part of the C ABI of libisac_hip.so under ISAC_ABI_VERSION 8 (two new entry points; no new struct,
 * no new isac_abi_sizeof selector; nothing that include/isac.h or the other additive headers declare changes).  Included by isac.h: include that.  Conventions: isac.h.
 *
 * fft2D detects on every antenna plane by itself (fft2D.m:59-96), and the per-target lists (isac_targets.h, isac_targets_upa.h) pair what those per-antenna lists hold:
 * an echo that no single element lifts over its CFAR threshold does not exist for them, however wide the array.  The calls here combine the array coherently BEFORE the
 * detector.  PROJECT-DEFINED, like the lists and the detectors of isac_cfar.h.  Indices are 1-based.  Input: what the LAST COMPLETED
 * isac_fft2d[_dev] / isac_fft2d_collect left on the device -- the range rows, the window geometry and the stored isac_cfar_config.
 *   1. complex window   Y[r,c,a] = rdm(r,c,a) on every cell of the power window (nr x nc, halo included): the value step 3 of isac_fft2d_get_targets forms for a cell, by the
 *                       same multiply-add chain -- the min(L, nFFT) symbols of range row r in four quarters, symbol half-swap, twiddle index stepped by the Doppler bin
 *                       modulo nFFT, (q0 + q1) + (q2 + q3), divided by sqrt(nFFT).  One device definition serves both: the lists' snapshots equal Y at their cells bit for bit.
 *   2. beam planes      Z[r,c,b] = sum_a conj(W[a,b]) Y[r,c,a], accumulated in ascending a from 0 with fp64 fused multiply-adds; Pb[r,c,b] = (re^2 + im^2) / n_b with
 *                       n_b = sum_a |W[a,b]|^2 (host, fp64, ascending a from 0.0): two rounded products, one rounded sum, one rounded division.  With this
 *                       normalisation a noise-only cell of a beam plane has the mean of a noise-only cell of an antenna plane, so the stored pfa and the 'Auto' factors
 *                       of isac_cfar.h apply unchanged; a matched beam gains A.
 *                       The matched weight of a direction is the element-wise SQUARE of its receive steering vector (the two-way phase of the path "transmit element a ->
 *                       receive element a").
 *   3. detection        detector m (isac_cfar.h), factor from the stored pfa or m->custom_factor, on every beam plane over the stored CUT rectangle with the stored guard /
 *                       training bands: the device code of isac_fft2d_redetect with the beam planes for the antenna planes.  Per-beam lists in CUT order (rows fastest) in
 *                       that call's format: det_idx, det_pow, beam_offsets [n_beams + 1], n_total; more detections than cap: ISAC_ERR_CAPACITY with n_total set.
 *   4. list             hits[r,c] = the number of beams whose list holds the cell; M[r,c] = max_b Pb[r,c,b], b* the first arg-max in ascending b (a NaN never wins).  A
 *                       target is a CUT cell with hits >= 1 whose M is strictly greater than the M of all 8 neighbours; a plateau gives none; a halo of 0 in either
 *                       dimension: ISAC_ERR_UNSUPPORTED.  Sorted by M descending, ties by ascending r + nIFFT (c-1); the strongest ISAC_MAX_TARGETS are returned, out->n_total
 *                       has the count.  out->power = M; out->hits, row, col, rng, vel as in isac_fft2d_get_targets; beam[i] = b* + 1; out->azi[i] = beam_azi[b*], or
 *                       b* + 1 where beam_azi is NULL.
 * ISAC_ERR_INVALID_ARG: W, m, out or beam NULL; n_beams < 1; a column of W with a zero or non-finite norm; a bad method block (the cases of isac_cfar2d); no completed
 * fft2D on the context, or -- rather than a stale answer -- a later call has rewritten its device state (the cases of isac_fft2d_get_targets).  ISAC_ERR_UNSUPPORTED:
 * n_beams > ISAC_MAX_BEAMS; nr nc n_beams >= 2^31; the detector limits of isac_fft2d_redetect; more than 4096 symbols.  ULA and UPA alike (W is the caller's); independent
 * of ISAC_OPT_UPA_DOA.  Both calls work in scratch of their own -- the power window, the detection lists, every other getter's answer, a pending submit and its result
 * buffer stay untouched -- run on the context's stream and return when complete.
 */
#ifndef ISAC_BEAMS_H
#define ISAC_BEAMS_H

#include "isac.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISAC_MAX_BEAMS 1024

/* Step 1 alone: the complex window of the LAST COMPLETED fft2D, Y[r,c,a] = rdm(r,c,a) on the cells of the power window.  Arguments and size query exactly as
 * isac_fft2d_get_power_window, with isac_c64 for double. */
int isac_fft2d_get_rdm_window(isac_ctx* ctx, isac_c64* Y, int64_t cap_elems, int32_t dims[3], int32_t* first_row, int32_t* first_col);

/* Steps 1-4.  W: host, [A x n_beams] column-major.  beam: [ISAC_MAX_TARGETS], 1-based.  beam_pow (optional): the beam planes, host [nr x nc x n_beams]. */
int isac_fft2d_beam_detect(isac_ctx* ctx, const isac_c64* W, int32_t n_beams, const double* beam_azi /* [n_beams] labels, or NULL */, const isac_cfar_method* m,
                           isac_target_list* out, int32_t* beam, int32_t* det_idx /* [2 x cap] or NULL */, double* det_pow /* [cap] or NULL */, int32_t cap,
                           int32_t* beam_offsets /* [n_beams+1] or NULL */, int32_t* n_total, double* beam_pow);

#ifdef __cplusplus
}
#endif
#endif /* ISAC_BEAMS_H */
