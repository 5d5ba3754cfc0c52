/*
 * isac_lazy_cov.h -- how the covariance of a NATIVE lazy echo grid is formed: an ADDITIVE part of the C ABI of libisac_hip.so under ISAC_ABI_VERSION 8 (two new entry
 * points, no new struct, no new isac_abi_sizeof selector, no new isac_ctx_set_option option; nothing that isac.h, isac_targets.h, isac_cfar.h or isac_cfar_mc.h declare
 * changes).  Included by isac.h: include that.  Conventions: isac.h.
 *
 * A native lazy echo grid is what isac_mono_static_sensing_fused_dev keeps inside the context when d_echo_grid == NULL on the spectral Philox route with 49..64 antennas and
 * one or two LoS targets: echoGrid[k, l, r] = sum_q D_q[k, l] a_q[r] + sig w[k, l, r].  isac_fft2d_submit_cached_dev with d_rx_grid == NULL needs its covariance
 * Ra = X X' / N (fft2D.m:106-107).  Both routes give the same estimates; Ra is equal to rounding (<= 1e-13 of the array form):
 *   ISAC_LAZY_COV_SPLIT (default)   N Ra = sig^2 W W' + sig (cross terms of w with D a) + a (D' D) a': the noise term W W' -- the whole MFMA bulk, a function of the seed and the
 *                                   shape alone -- is formed at the head of the fused call, in the kernel that streams txWaveform for the beam-sum; the fused range kernel adds
 *                                   the cross term; a small kernel assembles Ra in fft2D.  With two LoS targets the cross term is a pass of its own in fft2D.
 *   ISAC_LAZY_COV_REGENERATE        the beam-sum in a launch of its own, and one kernel in fft2D that re-forms the whole grid slab by slab from D, a and the seed.
 * The route is chosen in the fused call: set it before that call.  Any other value: ISAC_ERR_INVALID_ARG.
 */
#ifndef ISAC_LAZY_COV_H
#define ISAC_LAZY_COV_H

#include "isac.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { ISAC_LAZY_COV_SPLIT = 0, ISAC_LAZY_COV_REGENERATE = 1 };
int isac_ctx_set_lazy_cov_route(isac_ctx* ctx, int32_t route);
/* *route = the route the context's last covariance of a native lazy echo grid took (isac_fft2d_submit_cached_dev with d_rx_grid == NULL); ISAC_ERR_INVALID_ARG while there
 * has been none. */
int isac_ctx_get_lazy_cov_route_used(isac_ctx* ctx, int32_t* route);

#ifdef __cplusplus
}
#endif

#endif /* ISAC_LAZY_COV_H */
