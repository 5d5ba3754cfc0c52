/*
 * isac_directions.h -- off-grid direction finding with several sources per array snapshot: an ADDITIVE part of the C ABI of libisac_hip.so under ISAC_ABI_VERSION 8 (one new
 * entry point; no new struct, no new isac_abi_sizeof selector; nothing that include/isac.h or the other additive headers declare changes).  Included by isac.h: include
 * that.  Conventions: isac.h.
 *
 * The lists (isac_fft2d_get_targets[_upa], isac_fft2d_beam_detect, isac_fft2d_refine_targets, isac_fft2d_clean_targets) read a direction off the 1-degree grids of music.m:
 * the first arg-max of a Bartlett scan.  That leaves a quantisation floor of about 0.29 degrees rms, misses the main lobe of a 256-element array (its half width is 1/A =
 * 0.0039 in d sind(phi); a degree at boresight is 0.0087), and gives ONE direction per range-Doppler cell however many targets share the cell.  This call works on the array
 * snapshots those lists return (their `snapshots` argument): per snapshot, up to max_sources directions OFF the grid, by a greedy search with a joint re-fit (RELAX: Li and
 * Stoica 1996).  PROJECT-DEFINED.  It needs no completed fft2D.
 *
 * DIRECTION PARAMETERS: the spatial frequencies the project's steering vectors are functions of, d = 0.5 wavelengths, A = the number of elements.
 *   ULA   a[m] = exp(-2 pi j m f), f = d sind(phi); B_r(f) = |sum_m r[m] e^{+2 pi j m f}|^2 = |a(f)^H r|^2, periodic in f with period 2 d.  dir_u = f / d; dir_v and ele
 *         are not written and may be NULL.  One LOBE on the axis is 1 / A in f.
 *   UPA   a[n + nH m] = exp(-2 pi j d (m u + n v)), nH = n_ants_y, m < n_ants_x, n < nH; u = sind(theta) cosd(phi), v = sind(theta) sind(phi); B_r(u, v) = |a(u, v)^H r|^2 on
 *         the visible disc u^2 + v^2 <= 1.  dir_u = u, dir_v = v.  One lobe is 1 / (d n_ants_x) in u and 1 / (d n_ants_y) in v.
 * REPORTED ANGLES, the principal branch:  ULA azi = asind(dir_u) in [-90, 90];  UPA ele = asind(min(1, hypot(u, v))) in [0, 90], azi = atan2d(v, u).  The lists report
 * whichever mirror twin has the lower grid index -- 180 - phi for the ULA, (-theta, phi -+ 180) for the UPA: the two agree in dir_u, dir_v and not necessarily in degrees.
 *
 * FOR ONE ENTRY x (a column of `snapshots`), K = max_sources, every value in fp64, every phasor the sincos of its full argument (never a recurrence):
 *   1. greedy pass, k = 0 .. K-1
 *      residual    r = x - sum_{j<k} alpha_j a(p_j)
 *      coarse      the first arg-max of B_r over a uniform grid whose step h is a quarter of a lobe on every axis.  ULA: G = 4 A points f_g = -d + 2 d g / G.  UPA:
 *                  G_u x G_v = 4 n_ants_x x 4 n_ants_y points u = -1 + 2 g_u / G_u, v = -1 + 2 g_v / G_v; points with u^2 + v^2 > 1 are left out; index g_u + G_u g_v.  NaN
 *                  never wins, on a tie the lowest index wins.  A maximum that is 0 or NaN (no point wins) ends the pass: n_found = k.
 *      maximiser   on one axis, around a centre c with the other coordinate held: with g(t) = dB_r/dt (analytic: S = sum r e^{..}, D = sum m r e^{..}, g = -4 pi c_ax
 *                  Im(conj(S) D), c_ax = 1 for f and d for u, v), if g(c - h) > 0 > g(c + h) the zero of g in [c - h, c + h] by 40 halvings on the sign of g (g > 0: the
 *                  zero lies above), the midpoint of the last bracket; otherwise -- the box holds no interior maximum -- c stands.  The operation count does not depend on
 *                  the data.  ULA: p = that zero around the coarse point.  UPA: 3 rounds of (u at fixed v, then v at the new u), every round in the box around the SAME
 *                  centre; for a single source B is a product of a function of u and one of v and the first round is already exact.  A UPA result with u^2 + v^2 > 1 is
 *                  scaled by 1 / hypot(u, v) onto the disc; a ULA result outside [-d, d) is brought back by the period 2 d.
 *      amplitude   alpha_k = a(p_k)^H r / A
 *      RELAX       if k >= 1, `cycles` times: for j = 0 .. k in order  r_j = x - sum_{i != j} alpha_i a(p_i);  p_j = the maximiser of B_{r_j} in the box of one coarse
 *                  step around the current p_j;  alpha_j = a(p_j)^H r_j / A.
 *   2. order       the n_found sources by |alpha|^2 descending, ties in extraction order.  power = |alpha|^2.  n_src = the number of LEADING sources with |alpha_k|^2 >=
 *                  min_ratio |alpha_0|^2 and |alpha_k|^2 >= min_power.  All n_found are written (source k of entry i at k + max_sources i); the slots behind them hold NaN
 *                  (doubles) and 0 (amp).  residual = ||x - sum alpha a||^2 / A over all n_found sources.
 *   3. status      0: a normal entry.  1: nothing found (an all-zero snapshot, or one that holds a NaN): n_found = n_src = 0, residual = ||x||^2 / A.
 * The result of an entry is a function of its snapshot alone: no floating-point atomics, no dependence on the order of arrival or on the other entries.
 *
 * ISAC_ERR_INVALID_ARG: a NULL ep, status, n_found, n_src, azi, dir_u or power, a NULL snapshots with n > 0; a planar array (ep->array_is_upa) without ele or dir_v; n < 0
 * or n > ISAC_MAX_TARGETS; max_sources outside 1 .. min(ISAC_DIR_MAX_SOURCES, A - 1); cycles < 0; min_ratio outside [0, 1] or not finite; min_power negative or not
 * finite; A < 2; for a planar array n_ants_x n_ants_y != A (or either below 1).  ISAC_ERR_UNSUPPORTED: more than 256 elements.  Arguments are checked before any device work
 * and a refused call writes nothing; n == 0 returns ISAC_OK.  Of ep only array_is_upa, n_ants_x and n_ants_y are read.  Runs on the context's stream in scratch of its own
 * and returns when complete; every getter's answer, the state of the last CPI, a pending submit and its result buffer stay untouched.
 *
 * LIMITS: two sources closer than about a lobe are not separated (the greedy start lands between them); the number of sources is the caller's (max_sources, min_ratio,
 * min_power: no noise model in the library); the range stays on its grid; fft2D's own aziEst / eleEst do not use this call; no MEX command.
 */
#ifndef ISAC_DIRECTIONS_H
#define ISAC_DIRECTIONS_H

#include "isac.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISAC_DIR_MAX_SOURCES 8
#define ISAC_DIR_CYCLES 16          /* defaults of sensing.estimation.resolveDirections */
#define ISAC_DIR_MIN_RATIO 0.01

int isac_resolve_directions(isac_ctx* ctx, const isac_est_params* ep,
                            const isac_c64* snapshots /* [A x n], host, column i = entry i */, int32_t A, int32_t n,
                            int32_t max_sources, int32_t cycles, double min_ratio, double min_power,
                            int32_t* status, int32_t* n_found, int32_t* n_src /* [n] each */,
                            double* azi, double* ele, double* dir_u, double* dir_v, double* power /* [max_sources x n] each, source k of entry i at k + max_sources i */,
                            isac_c64* amp /* [max_sources x n] or NULL */, double* residual /* [n] or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* ISAC_DIRECTIONS_H */
