/*
 * isac_localize.h -- multi-static localisation: the per-link lists of several (transmitter, receiver) pairs fused into one position and one velocity vector per target, in
 * the network frame: an ADDITIVE part of the C ABI of libisac_hip.so under ISAC_ABI_VERSION 8 (two new entry points; no new struct, no new isac_abi_sizeof selector: flat
 * arrays; nothing that include/isac.h or the other headers declare changes).  STAND-ALONE: this header includes isac.h and is NOT included by it.  Conventions: isac.h.
 * PROJECT-DEFINED (the reference is mono-static only).  fp64 everywhere.
 *
 * ---- THE SCENE, the same arguments in the same order in both calls (host arrays):
 *   nodes [N x 3]     x, y, z of node n at nodes[3 n ..], metres, in the frame of gNBPosition.
 *   link_tx, link_rx [K]   the (tx node, rx node) of link k; tx == rx is a mono-static link.
 *   meas_link [M]     the link of measurement m, ASCENDING (the measurements are stored sorted by link; the Python wrapper sorts stably).
 *   meas_r [M]        range sum R_tx + R_rx, metres (2 rng of a mono-static list).
 *   meas_s [M]        Doppler sum v_tx + v_rx, m/s, "approaching" positive (2 vel of a list); NaN = none.
 *   meas_azi [M]      azimuth in degrees seen from the rx node, atan2(y - y_rx, x - x_rx); NaN = not used.
 *   sigma_r, sigma_v, sigma_a [M]   all > 0.
 *   grid              x = x0 + ix dx, ix = 0 .. nx - 1; y = y0 + iy dy, iy = 0 .. ny - 1; on the plane of height z.  Distances are 3-D.  Flat index iy nx + ix (x fastest).
 * For grid point g and measurement m of link (tx, rx):
 *     rho   = |g - p_tx| + |g - p_rx| - r_m
 *     alpha = wrap(azi_rx(g) - azi_m) into [-180, 180),  azi_rx(g) = atan2(y - y_rx, x - x_rx) in degrees (0 where both differences are 0)
 *     q     = (rho / sigma_r)^2 + (alpha / sigma_a)^2, the second term absent for a NaN azimuth
 *     w     = exp(-q / 2)
 *
 * ---- A. isac_position_map_dev: d_map [ny x nx] (device), S(g) = sum over links k = 0 .. K - 1, ascending, of max_{m in link k} w_m(g); a link without a measurement adds 0.
 * The maximum of a link is formed as exp(-min_m q_m / 2): one exponential per (point, link).  One thread owns one grid point and sums its links itself: no cross-thread
 * reduction and no atomics, so a point's value is the same bits on every run, for any grid around it.  The call runs on the context's stream and returns when complete.
 * With isac_profile_enable(ctx, 1) the event pair of isac_profile_last_kernel_ms brackets the map kernel.
 *
 * ---- B. isac_localize_dev: peaks of ANY device map [ny x nx] (A's, or the caller's own), then the greedy claim that removes ghosts.
 *   candidates   cell c is a candidate when map[c] >= min_score and, for each of its (up to 8) neighbours n inside the grid, map[c] > map[n] where n < c (flat index) and
 *                map[c] >= map[n] where n > c.  Sorted by map value descending, then flat index ascending; the first max_cand are kept.
 *   per candidate, in that order:
 *     1. associate   at the cell centre each link takes, among its measurements no accepted target has claimed, the one with the smallest q (lowest m on a tie) and
 *                    keeps it if q <= gate^2.
 *     2. fewer than min_links links kept: status 1.
 *     3. refine      iters Gauss-Newton steps on (x, y) for sum (rho / sigma_r)^2 + (alpha / sigma_a)^2 over the kept measurements (fixed during the steps): rows
 *                    J = d(rho)/d(x, y) / sigma_r = (u_tx + u_rx)_xy / sigma_r and d(alpha)/d(x, y) / sigma_a = (180 / pi) (-e_y, e_x) / (e_x^2 + e_y^2) / sigma_a, e = g - p_rx,
 *                    u_n the 3-D unit vector from node n to g; H = sum J^T J and b = sum J^T res summed in link order; step = -H^-1 b.
 *     4. at any step not (det H > 1e-12 (tr H / 2)^2): status 2.  After the steps not (|final - cell centre| <= max_move): status 3.
 *     5. otherwise accepted.  The first max_targets accepted ones get status 0, are written out and claim their measurements; later ones get status 4 and claim nothing.
 *     6. velocity    of an accepted target, at the final point: the least-squares solution of s_m / sigma_v = -v . (u_tx + u_rx)_xy / sigma_v over the kept measurements with a
 *                    finite s (normal equations summed in link order).  Fewer than 2 of them, or not (lambda_min / lambda_max >= 1e-8) of the 2 x 2 normal matrix
 *                    (lambda = h -+ sqrt(((n11 - n22) / 2)^2 + n12^2), h = (n11 + n22) / 2): vel = NaN, vel_status = 1.
 *   outputs (host), for target t = 0 .. n_out[0] - 1 in order of acceptance: pos[2 t ..] = x, y; vel[2 t ..]; vel_status[t]; score[t] = the map at the candidate's cell;
 *   n_links[t]; assoc[K t + k] = the measurement of link k (an index into the M given) or -1; rms[t] = sqrt(sum q / n_links) at the final point.  For candidate
 *   c = 0 .. n_out[1] - 1, where the arrays are not NULL: cand_cell[c] (flat index), cand_score[c], cand_status[c].  n_out[0] = targets, n_out[1] = candidates.  Nothing
 *   beyond n_out[0] (n_out[1]) entries of an output is written.
 * DETERMINISM.  The candidate list is the top max_cand of a strict total order (value, index): whatever the schedule.  The greedy stage is one workgroup.
 *
 * LIMITS, otherwise ISAC_ERR_INVALID_ARG before any device work, nothing written: 1 <= N <= 64; 1 <= K <= 256; 1 <= M <= 4096; 1 <= nx, ny <= 8192 and nx ny <= 2^26;
 * 1 <= max_cand, max_targets <= 256; 0 <= iters <= 64; min_links >= 0; node positions, r, the sigmas, x0, y0, dx, dy, z finite (B: min_score, gate and max_move too);
 * sigmas, dx, dy > 0; an azimuth finite or NaN; a link's node index in 0 .. N - 1; meas_link in 0 .. K - 1 and ascending; no NULL scene array, map or (B) target output or n_out.
 * SCRATCH.  The context's own (tables, per-block candidate lists, the outputs' device copies).  Both calls leave the last CPI, cached range rows, every getter's answer and
 * a pending submit untouched.
 *
 * OUT OF SCOPE: a 3-D position search; elevation; a joint re-fit of all targets; tracking across CPIs; a MEX command.
 */
#ifndef ISAC_LOCALIZE_H
#define ISAC_LOCALIZE_H

#include "isac.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISAC_LOCALIZE_MAX_NODES 64
#define ISAC_LOCALIZE_MAX_LINKS 256
#define ISAC_LOCALIZE_MAX_MEAS 4096
#define ISAC_LOCALIZE_MAX_SIDE 8192
#define ISAC_LOCALIZE_MAX_CELLS (1 << 26)
#define ISAC_LOCALIZE_MAX_CAND 256
#define ISAC_LOCALIZE_MAX_ITERS 64

int isac_position_map_dev(isac_ctx* ctx, const double* nodes /* [N x 3] */, int32_t n_nodes, const int32_t* link_tx, const int32_t* link_rx /* [K] */, int32_t n_links,
                          const int32_t* meas_link, const double* meas_r, const double* meas_s, const double* meas_azi, const double* sigma_r, const double* sigma_v,
                          const double* sigma_a /* [M] each */, int32_t n_meas, double x0, double dx, int32_t nx, double y0, double dy, int32_t ny, double z,
                          double* d_map /* [ny x nx], device */);

int isac_localize_dev(isac_ctx* ctx, const double* nodes /* [N x 3] */, int32_t n_nodes, const int32_t* link_tx, const int32_t* link_rx /* [K] */, int32_t n_links,
                      const int32_t* meas_link, const double* meas_r, const double* meas_s, const double* meas_azi, const double* sigma_r, const double* sigma_v,
                      const double* sigma_a /* [M] each */, int32_t n_meas, double x0, double dx, int32_t nx, double y0, double dy, int32_t ny, double z,
                      const double* d_map /* [ny x nx], device */, double min_score, int32_t max_cand, int32_t min_links, double gate, int32_t iters, double max_move,
                      int32_t max_targets, double* pos /* [2 x max_targets] */, double* vel /* [2 x max_targets] */, int32_t* vel_status, double* score, int32_t* n_links_out,
                      int32_t* assoc /* [K x max_targets] */, double* rms, int32_t* cand_cell, double* cand_score, int32_t* cand_status /* [max_cand] each, or NULL */,
                      int32_t* n_out /* [2] */);

#ifdef __cplusplus
}
#endif
#endif /* ISAC_LOCALIZE_H */
