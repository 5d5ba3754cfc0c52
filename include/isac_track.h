/*
 * isac_track.h -- target tracking across CPIs: banks of constant-velocity Kalman tracks that live on the device and take, scan after scan, position fixes (a
 * localizeTargets result) and per-link measurements (range sum, azimuth, Doppler sum): an ADDITIVE part of the C ABI of libisac_hip.so under ISAC_ABI_VERSION 8 (four new
 * entry points; no new struct, no new isac_abi_sizeof selector: flat arrays; nothing that include/isac.h or the other headers declare changes).  STAND-ALONE: this header
 * includes isac.h and is NOT included by it.  Conventions: isac.h.  PROJECT-DEFINED (the reference is single-CPI).  fp64 everywhere.
 *
 * ---- BANKS AND THE STATE BLOCK.  A bank is an independent tracker (a cell, a Monte-Carlo drop) of T = max_tracks slots; the B = n_banks banks of a state block share the
 * scene and the parameters of a call and nothing else.  The block is device memory of isac_track_state_bytes(B, T) bytes that the CALLER owns (isac_dev_alloc); its layout is
 * the library's.  A slot holds
 *   status   0 free, 1 tentative, 2 confirmed            id   per bank 1, 2, 3 .. in order of birth, never reused            age, hits, misses
 *   x [4]    (x, y, vx, vy) in the frame of `nodes`, on the plane z = height            P [4 x 4]   row-major, exactly symmetric
 *   nis, dof   the sum of the d^2 applied to the slot in the last scan and the number of their components (for consistency checks)
 * and a bank holds the id it gave last.  isac_track_reset_dev: every slot free (all fields 0), every bank's id counter 0.
 *
 * ---- THE SCENE (host arrays), with the meaning of isac_localize.h: nodes [N x 3]; link_tx, link_rx [K], the (tx node, rx node) of link k; height.
 * ---- THE MEASUREMENTS (host arrays).  Bank b owns measurements bank_first[b] .. bank_first[b + 1] - 1; bank_first[0] = 0, M = bank_first[B] (0 is allowed).
 *   meas_group [M]   the group, 0 .. ISAC_TRACK_MAX_GROUPS - 1, ASCENDING inside a bank (the Python wrapper sorts stably).  A group is one sensor's view of the scan: one link's
 *                    list, or one localizeTargets result.  Group numbers nobody uses cost nothing.
 *   meas_kind [M]    0 = fix, 1 = link.            meas_link [M]   the link of a kind-1 measurement, 0 .. K - 1 (not read for kind 0).
 *   meas_z [M x 4]   kind 0: x, y, vx, vy (x, y finite; vx, vy finite or NaN = absent).  kind 1: r, azi, s, unused (range sum R_tx + R_rx in metres, finite; azimuth in
 *                    degrees seen from the rx node, finite or NaN = absent; Doppler sum v_tx + v_rx in m/s, "approaching" positive, finite or NaN = absent).
 *   meas_sigma [M x 4]   the standard deviations of the same components, all four finite and > 0 (also those of absent or unused components).
 *
 * ---- isac_track_step_dev: ONE SCAN of every bank.
 *   1. predict every live slot:  x <- F x,  P <- F P F^T + Q,  then P_ij = P_ji = (P_ij + P_ji) / 2;  F = [[1, 0, dt, 0], [0, 1, 0, dt], [0, 0, 1, 0], [0, 0, 0, 1]],
 *      Q = sigma_acc^2 [[dt^4/4, 0, dt^3/2, 0], [0, dt^4/4, 0, dt^3/2], [dt^3/2, 0, dt^2, 0], [0, dt^3/2, 0, dt^2]].  dt = 0 is allowed.  Every slot's nis and dof start the scan at 0.
 *   2. the bank's groups in ascending order.  Inside a group a track takes at most one measurement and a measurement goes to at most one track; across groups a track may
 *      take several, and group g sees the states that the groups below it have updated.
 *   3. a measurement is up to four scalar COMPONENTS applied in a fixed order, each linearised at the state the components before it have left (a sequential scalar EKF):
 *        kind 0   x, y, vx, vy: prediction = the state's component, row H = the unit vector.
 *        kind 1   range sum:    prediction |p - p_tx| + |p - p_rx|, p = (x, y, height); H = (g_x, g_y, 0, 0), g = (u_tx + u_rx)_xy, u_n the 3-D unit vector from node n to p
 *                               (the zero vector where the distance is 0).
 *                 azimuth:      e = (x - x_rx, y - y_rx); SKIPPED where e_x^2 + e_y^2 = 0; prediction atan2(e_y, e_x) in degrees, the innovation wrapped into [-180, 180)
 *                               (w - 360 floor((w + 180) / 360)); H = (180 / pi) (-e_y, e_x, 0, 0) / (e_x^2 + e_y^2).
 *                 Doppler sum:  prediction -(vx g_x + vy g_y), g formed anew at the current state; H = (0, 0, -g_x, -g_y).  The dependence of g on the position is
 *                               DELIBERATELY left out of the row: a Doppler sum corrects the velocity only.
 *      one component with innovation nu = measured - predicted and variance sigma^2:
 *        PH_i = sum_j P_ij H_j (j ascending);  s = sum_i H_i PH_i + sigma^2;  K = PH / s;  x += K nu;  P_ij -= K_i PH_j;  P_ij = P_ji = (P_ij + P_ji) / 2.
 *      The DISTANCE of a (track, measurement) pair is d^2 = sum nu^2 / s over its components along a VIRTUAL update of a copy of the track, and its component count the
 *      number of components applied (absent and skipped ones do not count).  For kind 0 (H rows of I, R diagonal) d^2 is the joint Mahalanobis distance.
 *   4. association in a group, greedy, best first: among the pairs (live track without a measurement of this group, measurement of the group nobody has taken) the one with
 *      the smallest d^2 <= gate^2 is taken -- a tie goes to the lower slot, then to the lower measurement index -- and the update is applied for real (nis += d^2,
 *      dof += its component count); repeat until no pair qualifies.  The d^2 of other tracks do not change when one track is updated.  Optimal assignment is out of scope.
 *   5. bookkeeping, after the bank's last group: every live track age += 1; with at least one measurement in the scan hits += 1 and misses = 0, otherwise misses += 1;
 *      a tentative track with hits >= confirm_hits becomes confirmed; then a tentative track with misses >= tent_misses and a confirmed track with misses >= max_misses is
 *      freed (status 0; the other fields keep the values they have by then).
 *   6. births: every kind-0 measurement left without a track starts a tentative track, in measurement order, in the lowest free slot (a slot freed in this scan counts):
 *      x = (x, y, vx or 0, vy or 0), P = diag(sigma_x^2, sigma_y^2, sigma_vx^2 or init_v0^2, sigma_vy^2 or init_v0^2) ("or": where the component is NaN), hits = 1,
 *      misses = 0, age = 1, nis = 0, dof = 0, the bank's next id.  With no free slot left the measurement is marked "table full" and nothing else changes.  Kind-1
 *      measurements never start a track (one-point initiation from a link is out of scope).
 *   outputs (host): the TABLE, [B x T] each: status, id, age, hits, misses, x [B x T x 4], P [B x T x 16], nis, dof -- the state block as the scan left it;
 *   per measurement assoc [M] (the slot, or -1) and assoc_kind [M] (0 none, 1 updated a track, 2 born, 3 table full); n_confirmed [B].
 * ---- isac_track_get_dev: the table of the state block as it stands; it does not step.
 * DETERMINISM.  One workgroup per bank, one thread per slot, a strict total order (d^2, slot, measurement) in every round, no atomics, nothing shared between banks:
 * the result is a function of the inputs alone and two runs give the same bits.
 *
 * LIMITS, otherwise ISAC_ERR_INVALID_ARG before any device work, the state and every output untouched: 1 <= B <= 1024; 1 <= T <= 256; 1 <= N <= 64; 1 <= K <= 256;
 * 0 <= M <= 2^20; at most 256 measurements in a group; bank_first[0] = 0 and not descending; meas_group in 0 .. 255 and ascending inside a bank; meas_kind 0 or 1; the link
 * of a kind-1 measurement in 0 .. K - 1; a link's node index in 0 .. N - 1; node positions, height, dt, sigma_acc, gate, init_v0 finite; dt >= 0; sigma_acc >= 0;
 * confirm_hits, tent_misses, max_misses >= 1; the values and sigmas as stated above; no NULL state, scene array, bank_first, table output or n_confirmed; the measurement
 * arrays and assoc, assoc_kind may be NULL only where M = 0.  isac_track_state_bytes returns 0 for B or T outside their limits.
 * SCRATCH.  The context's own (the scene's tables, the measurements, the outputs' device copies).  The calls run on the context's stream and return when complete; they
 * leave the last CPI, cached range rows, every getter's answer and a pending submit untouched.  With isac_profile_enable(ctx, 1) the event pair of
 * isac_profile_last_kernel_ms brackets the step kernel.
 *
 * OUT OF SCOPE: optimal assignment; M-of-N confirmation; initiation from link measurements; manoeuvre models / IMM; a 3-D state; a MEX command.
 */
#ifndef ISAC_TRACK_H
#define ISAC_TRACK_H

#include "isac.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISAC_TRACK_MAX_BANKS 1024
#define ISAC_TRACK_MAX_TRACKS 256
#define ISAC_TRACK_MAX_GROUPS 256
#define ISAC_TRACK_MAX_GROUP_MEAS 256
#define ISAC_TRACK_MAX_MEAS (1 << 20)
#define ISAC_TRACK_MAX_NODES 64
#define ISAC_TRACK_MAX_LINKS 256

int64_t isac_track_state_bytes(int32_t n_banks, int32_t max_tracks);

int isac_track_reset_dev(isac_ctx* ctx, void* d_state, int32_t n_banks, int32_t max_tracks);

int isac_track_step_dev(isac_ctx* ctx, void* d_state, int32_t n_banks, int32_t max_tracks, const double* nodes /* [N x 3] */, int32_t n_nodes, const int32_t* link_tx,
                        const int32_t* link_rx /* [K] */, int32_t n_links, double height, double dt, double sigma_acc, double gate, int32_t confirm_hits, int32_t tent_misses,
                        int32_t max_misses, double init_v0, const int32_t* bank_first /* [B + 1] */, const int32_t* meas_group, const int32_t* meas_kind,
                        const int32_t* meas_link /* [M] each */, const double* meas_z, const double* meas_sigma /* [M x 4] each */, int32_t* status, int32_t* id, int32_t* age,
                        int32_t* hits, int32_t* misses /* [B x T] each */, double* x /* [B x T x 4] */, double* P /* [B x T x 16] */, double* nis, int32_t* dof /* [B x T] each */,
                        int32_t* assoc, int32_t* assoc_kind /* [M] each */, int32_t* n_confirmed /* [B] */);

int isac_track_get_dev(isac_ctx* ctx, const void* d_state, int32_t n_banks, int32_t max_tracks, int32_t* status, int32_t* id, int32_t* age, int32_t* hits,
                       int32_t* misses /* [B x T] each */, double* x /* [B x T x 4] */, double* P /* [B x T x 16] */, double* nis, int32_t* dof /* [B x T] each */);

#ifdef __cplusplus
}
#endif
#endif /* ISAC_TRACK_H */
