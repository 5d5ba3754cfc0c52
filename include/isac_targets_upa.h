/*
 * isac_targets_upa.h -- the per-target list of fft2D for a uniform planar array: an ADDITIVE part of the C ABI of libisac_hip.so under ISAC_ABI_VERSION 8 (one new entry
 * point; no new struct, no new isac_abi_sizeof selector; nothing that include/isac.h or include/isac_targets.h declares changes).  Included by isac.h: include that.
 * Conventions: isac.h.
 */
#ifndef ISAC_TARGETS_UPA_H
#define ISAC_TARGETS_UPA_H

#include "isac.h"

#ifdef __cplusplus
extern "C" {
#endif

/* isac_fft2d_get_targets (isac_targets.h) for a UPA context: paired (range, velocity, azimuth, elevation) entries of the LAST COMPLETED isac_fft2d[_dev] /
 * isac_fft2d_collect on this context.  PROJECT-DEFINED, like that call; it reuses isac_target_list and adds the elevations in an array of the caller's.
 * Steps 1, 2, 3 and 5 are those of isac_fft2d_get_targets, word for word -- the integrated map S, the hits, the strict 8-neighbour maximum, the snapshot
 * x[r] = rdm(row, col, r), the order, rng, vel, n_total, the ISAC_MAX_TARGETS cut and ISAC_ERR_CAPACITY do not depend on the array type, and one device code produces them
 * for both calls: on the same echo grid the two lists agree in every one of those fields, bit for bit.
 *   4. direction (UPA)  B(j) = |sum_r conj(a_j[r]) x[r]|^2 over the eSteps x aSteps scan grid of music.m:36-53 (181 x 361 points by default), j = e + eSteps a
 *                       (column-major, 0-based), with the steering vector of the 2-D DoA scan (music.m:44-55):
 *                           a_j[r] = exp(-2j pi sind(th_e) (m d cosd(ph_a) + n d sind(ph_a))),  d = 0.5,  element r = n + n_ants_y m,  m < n_ants_x,  n < n_ants_y
 *                       (th_e = e eGran - eMax/2, ph_a = a aGran - aMax/2; the same table and the same expression, in the same association, as isac_music_doa's UPA
 *                       branch).  The target's direction is the FIRST index j of the maximum: azi = ph_a, ele[t] = th_e (music.m:70-71).  The mirror twins
 *                       (-th, ph -+ 180) have bitwise equal steering vectors and therefore bitwise equal B: every direction ties with its twin and the lower j is
 *                       reported, as for the ULA list and for MUSIC.  The result is a function of the snapshots alone (no floating-point atomics, no order of arrival).
 * out->azi is filled; ele[0 .. n_targets-1] is written (ele holds ISAC_MAX_TARGETS doubles).  snapshots / cap_snap: as isac_fft2d_get_targets.
 * ISAC_ERR_INVALID_ARG: out or ele NULL; no completed fft2D on the context, or a later call has rewritten its device state (the rule of isac_fft2d_get_targets);
 * n_ants_x n_ants_y of that fft2D's isac_est_params is not its antenna count.  ISAC_ERR_UNSUPPORTED: a ULA context (isac_fft2d_get_targets is its list); a halo of 0 in
 * either dimension; more than 256 elements (the limit of the 2-D scan).
 * The call does NOT depend on ISAC_OPT_UPA_DOA: it needs the range rows, the power window and the CFAR lists only, and a UPA fft2D leaves those on the context also when
 * its own DoA stage answered ISAC_ERR_UNSUPPORTED (option off) -- the list is returned then, and it is the same list, byte for byte, with the option on.
 * Runs on the context's stream and returns when the list is complete; leaves the result of every other getter (isac_get_angular_spectrum2d among them), a pending submit
 * and its result buffer untouched. */
int isac_fft2d_get_targets_upa(isac_ctx* ctx, isac_target_list* out, double* ele /* [ISAC_MAX_TARGETS] */,
                               isac_c64* snapshots /* [A x cap_snap] or NULL */, int32_t cap_snap);

#ifdef __cplusplus
}
#endif
#endif /* ISAC_TARGETS_UPA_H */
