/*
 * isac_cfar.h -- the other detectors of phased.CFARDetector2D: an ADDITIVE part of the C ABI of libisac_hip.so under ISAC_ABI_VERSION 8 (three new entry points, one new
 * struct, one new isac_abi_sizeof selector; nothing that include/isac.h declares changes).  Included by isac.h: include that.  Conventions: isac.h.
 *
 * sensing.detection.cfar2D configures the detector with Method 'CA' and names the alternatives in the same line ('CA', 'GOCA', 'SOCA', 'OS'; cfar2D.m:28), and
 * ThresholdFactor 'Auto' ('Auto', 'Input port', 'Custom'; cfar2D.m:29).  The fft2D pipeline of isac.h stays cell averaging with the automatic factor; the entry points here
 * run any of the four on an arbitrary map, or again on the power window the last completed fft2D left on the device.  PROJECT-DEFINED where the toolbox does not say
 * (DESIGN.md section 5).  For a CUT at (r, c), hr = guard[0] + train[0], hc = guard[1] + train[1]:
 *   training cells  T_1 .. T_N: the (2 hr + 1) x (2 hc + 1) window around the CUT minus the (2 guard[0] + 1) x (2 guard[1] + 1) guard block, in the order in which the CA
 *                   detector adds them: column offset slowest, row offset fastest.  N is even.
 *   CA              noise = (T_1 + .. + T_N) / N, added from 0.0 in that order with correctly rounded fp64 operations: isac_cfar2d_ca, bit for bit.
 *   GOCA / SOCA     front half T_1 .. T_{N/2} (the cells before the CUT in that order: the columns left of the CUT and the upper part of its own column), rear half the
 *                   rest; each half is added from 0.0 in order and divided by N/2; noise = the greater (GOCA) / the smaller (SOCA) of the two means.
 *   OS              noise = the rank-th smallest training cell, 1 <= rank <= N.
 *   all             thr = alpha * noise (one correctly rounded multiply); detection iff P[cut] > thr, strict.  A NaN in the CUT or in ANY training cell: no detection.
 *   alpha           custom_factor > 0: that value ('Custom').  custom_factor == 0 ('Auto'): the root of the method's false-alarm equation in white Gaussian noise
 *                   (square-law detector, exponential cells), n = N/2, T = alpha / n:
 *                     CA    (1 + alpha/N)^-N = Pfa                                  -- the closed form N (Pfa^(-1/N) - 1) of isac_cfar2d_ca, the same double
 *                     SOCA  2 sum_{k=0}^{n-1} C(n-1+k, k) (2 + T)^-(n+k) = Pfa
 *                     GOCA  2 (1 + T)^-n - [the SOCA sum] = Pfa
 *                     OS    prod_{i=0}^{rank-1} (N - i) / (N - i + alpha) = Pfa
 *                   solved on the host in fp64: the bracket [0, 1] is doubled until it holds the root, then halved until its ends are adjacent doubles (or 200 times);
 *                   the upper end is returned.
 * Limits: GOCA / SOCA / OS accept N <= ISAC_CFAR_MAX_TRAIN training cells (the OS selection costs N^2 comparisons per CUT, and the SOCA series leaves the fp64 range
 * beyond it): more is ISAC_ERR_UNSUPPORTED.  CA has the limits of isac_cfar2d_ca.  ISAC_ERR_INVALID_ARG: an unknown method, rank outside 1..N (OS), custom_factor negative
 * or NaN, pfa outside (0, 1) with custom_factor == 0.
 */
#ifndef ISAC_CFAR_H
#define ISAC_CFAR_H

#include "isac.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { ISAC_CFAR_CA = 0, ISAC_CFAR_GOCA = 1, ISAC_CFAR_SOCA = 2, ISAC_CFAR_OS = 3 };
#define ISAC_CFAR_MAX_TRAIN 1024
typedef struct { int32_t method; int32_t rank;      /* OS only, 1..N; ignored otherwise                     */
                 double custom_factor;               /* 0 = 'Auto' (from pfa); > 0 = 'Custom'; else INVALID_ARG */ } isac_cfar_method;
#define ISAC_SIZEOF_CFAR_METHOD 12 /* isac_abi_sizeof selector of isac_cfar_method, behind ISAC_SIZEOF_TARGET_LIST; a library without it answers -1 */

/* The 'Auto' threshold factor of `method` for n_train training cells.  Host only: no context, no GPU. */
int isac_cfar_threshold_factor(int32_t method, int32_t n_train, int32_t rank, double pfa, double* alpha);

/* The phased.CFARDetector2D step on an arbitrary map and CUT list: isac_cfar2d_ca with the method block.  Same staging, CUT-list order, 1-based indices and errors
 * (ISAC_ERR_CFAR_WINDOW; ISAC_ERR_CAPACITY with n_det set).  method = ISAC_CFAR_CA with custom_factor = 0 gives isac_cfar2d_ca's output byte for byte. */
int isac_cfar2d(isac_ctx* ctx, const double* P, int32_t n_rows, int32_t n_cols, const int32_t* cut_idx, int32_t n_cut,
                const int32_t guard[2], const int32_t train[2], double pfa, const isac_cfar_method* m,
                int32_t* det_idx, int32_t cap, int32_t* n_det);

/* The LAST COMPLETED isac_fft2d[_dev] / isac_fft2d_collect on this context, detected again with another detector.  Reads the |rdm|^2 window [nr x nc x A], the
 * isac_est_params and the isac_cfar_config (guard, training, CUT rectangle, pfa) that call left in the context, runs detector `m` on every antenna plane over the CUT
 * rectangle, and then the host half of fft2D.m:63-99 on the new lists (peak sort per antenna, concatenation, the two unique(.,'stable')): out->rng_est / vel_est / n_rng /
 * n_vel / num_dets / total_detections.  out->n_azi = 0 and azi_est / ele_est are not filled: direction comes from isac_fft2d_get_covariance + isac_music_doa(num_dets, ..),
 * as in fft2D.m:110-111 -- so a UPA is accepted.  The per-antenna lists come back in CUT order (rows fastest) in the format of isac_fft2d_get_detections; more
 * detections than cap: ISAC_ERR_CAPACITY with n_total set.  Zero detections: ISAC_OK with empty lists.  ISAC_ERR_INVALID_ARG when there is no completed fft2D on the
 * context, and -- rather than a stale answer -- when a later call has rewritten the power window (the cases of isac_fft2d_get_targets).  Works in scratch of its own: the
 * power window, the detection lists and every other getter's answer, a pending submit and its result buffer stay untouched.  Runs on the context's stream and returns
 * when complete. */
int isac_fft2d_redetect(isac_ctx* ctx, const isac_cfar_method* m, isac_est_result* out,
                        int32_t* det_idx /* [2 x cap] or NULL */, double* det_pow /* [cap] or NULL */, int32_t cap,
                        int32_t* ant_offsets /* [A+1] or NULL */, int32_t* n_total);

#ifdef __cplusplus
}
#endif
#endif /* ISAC_CFAR_H */
