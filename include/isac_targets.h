/*
 * isac_targets.h -- the per-target list of fft2D: an ADDITIVE part of the C ABI of libisac_hip.so under ISAC_ABI_VERSION 8 (one new entry point, one new struct, one new
 * isac_abi_sizeof selector; nothing that include/isac.h declares changes).  Included by isac.h: include that.  Conventions: isac.h.
 */
#ifndef ISAC_TARGETS_H
#define ISAC_TARGETS_H

#include "isac.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-target list of the LAST COMPLETED isac_fft2d[_dev] / isac_fft2d_collect on this context: which range goes with which velocity and which direction.  fft2D itself
 * reports three unrelated lists (rngEst and velEst are de-duplicated independently, fft2D.m:99; aziEst comes from one covariance over the whole grid), while getRMSE.m:43-52
 * pairs them by index.  PROJECT-DEFINED, like isac_find2d_peaks (added under ABI 8: a new symbol and a new struct only).  Indices are 1-based.  Input: the range rows, the
 * |rdm|^2 window [nr x nc x A] and the per-antenna CFAR lists that call left on the device.
 *   1. integrated map   S[r,c] = sum_a P[r,c,a] over the power window, added in fp64 in ascending antenna order starting from 0.0; hits[r,c] = the number of antennas whose
 *                       CFAR list holds (r,c);
 *   2. target cells     a cell of the CUT zone with hits >= 1 whose S is strictly greater than the S of all 8 neighbours (the window carries a halo of guard + training
 *                       cells on each side, so the neighbours exist; a halo of 0 in either dimension: ISAC_ERR_UNSUPPORTED).  A plateau gives no target, NaN is never one;
 *   3. snapshot         x[a] = rdm(r,c,a), the complex value whose modulus the Doppler stage squares (fft2D.m:44-46: symbol half-swap, zero-pad or truncate to nFFT,
 *                       1/sqrt(nFFT), Doppler fftshift), as a single-bin DFT over the L symbols of range row r; antenna order unchanged;
 *   4. azimuth (ULA)    B(i) = |sum_m conj(a_i[m]) x[m]|^2, a_i[m] = exp(-2j pi m 0.5 sind(phi_i)) over the ULA scan grid of music.m:76-96 (361 angles by default, the
 *                       same sind table and steering expression as the MUSIC scan); azi = phi_i for the FIRST index of the maximum: mirror twins phi / 180 - phi are
 *                       bitwise equal, the lower index wins, as for MUSIC.  A UPA: ISAC_ERR_UNSUPPORTED, whatever ISAC_OPT_UPA_DOA says;
 *   5. order            S descending, ties by ascending column-major index r + nIFFT (c-1); rng = (r-1) rRes, vel = (c - nFFT/2 - 1) vRes (fft2D.m:77-82).
 * Expect more entries than physical targets: range and Doppler sidelobes that CFAR detects are local maxima too.
 * More than ISAC_MAX_TARGETS targets: the strongest ISAC_MAX_TARGETS are returned, n_total has the count.  snapshots (optional): x of target t at snapshots[a + A t];
 * more targets than cap_snap columns: ISAC_ERR_CAPACITY (n_total is set).  ISAC_ERR_INVALID_ARG when there is no completed fft2D on the context, and -- rather than a stale
 * answer -- when a later call has rewritten those buffers (isac_fft2d_range_stage_dev, a new fused echo call, a new submit, isac_ctx_reserve).  Runs on the context's
 * stream and returns when the list is complete; leaves the result of every other getter, a pending submit and its result buffer untouched. */
#define ISAC_MAX_TARGETS 1024
#define ISAC_SIZEOF_TARGET_LIST 11 /* isac_abi_sizeof selector of isac_target_list, behind the ISAC_SIZEOF_* enumerators of isac.h; a library without it answers -1 */
typedef struct { int32_t n_targets, n_total;
  int32_t row[ISAC_MAX_TARGETS], col[ISAC_MAX_TARGETS], hits[ISAC_MAX_TARGETS];
  double rng[ISAC_MAX_TARGETS], vel[ISAC_MAX_TARGETS], azi[ISAC_MAX_TARGETS], power[ISAC_MAX_TARGETS]; } isac_target_list;
int isac_fft2d_get_targets(isac_ctx* ctx, isac_target_list* out, isac_c64* snapshots /* [A x cap_snap] or NULL */, int32_t cap_snap);

#ifdef __cplusplus
}
#endif
#endif /* ISAC_TARGETS_H */
