/*
 * isac_beam_clean.h -- successive target cancellation (CLEAN) on beam planes of the last fft2D: an ADDITIVE part of the C ABI of libisac_hip.so under ISAC_ABI_VERSION 8 (one
 * new entry point; no new struct, no new isac_abi_sizeof selector; nothing that include/isac.h or the other additive headers declare changes).  Included by isac.h: include
 * that.  Conventions: isac.h.
 *
 * isac_fft2d_clean_targets (isac_clean.h) removes a strong echo's Doppler sidelobes, split lobes and gap lobes and uncovers a weaker echo under them -- but it detects per
 * antenna element, with no array gain.  isac_fft2d_beam_detect (isac_beams.h) has the array gain and lists echoes no single element lifts over its threshold -- but it reads
 * ONE map, so every beam plane carries the strong echo's sidelobes and a weak echo under them is hidden again.  This call is the loop of the first with the detector of the
 * second: an echo that needs BOTH the array gain and the removal of a stronger echo's Doppler response.  PROJECT-DEFINED.  Indices are 1-based;
 * parent[] holds 0-based entry indices.
 *
 * The call works on what the last completed fft2D left on the context (readiness and its errors: isac_fft2d_get_targets).  R is a copy of the window's range rows
 * ymid [nr x L x A] (natural symbol order) in scratch of the call's own; the rows themselves, the power window, the stored lists, every other getter's scratch (that of
 * isac_fft2d_beam_detect and of isac_fft2d_clean_targets included), a pending submit and its result buffer stay untouched.  W: host, [A x n_beams] column-major
 * (sensing.estimation.beamWeights gives matched columns).  For pass i = 0, 1, ...:
 *   1. planes     Y[r, c, a] = rdm(r, c, a) on every cell of the power window, formed from R by the chain of isac_fft2d_get_rdm_window (the single-bin DFT over the symbols
 *                 after the half swap, four quarters joined (q0 + q1) + (q2 + q3), / sqrt(nFFT)); Pb[r, c, b] from Y and W by step 2 of isac_beams.h: Z = sum_a conj(W[a, b])
 *                 Y[r, c, a] in ascending a from 0 with fp64 fused multiply-adds, Pb = (re^2 + im^2) / n_b with n_b = sum_a |W[a, b]|^2 (host, fp64, ascending a from 0.0) --
 *                 two rounded products, one rounded sum, one rounded division, never contracted.  A cell's value depends on its own row of R and on W and on nothing else.
 *   2. detect     step 3 of isac_beams.h: detector m with the stored isac_cfar_config (CUT zone, guard / training bands, pfa) on every beam plane.
 *   3. cells      step 4 of isac_beams.h: hits = the beams that detect the cell, M = max_b Pb, b* its first arg-max in ascending b (a NaN never wins); a cell is listed where
 *                 hits >= 1 and M is strictly greater than the M of all 8 neighbours; order by M descending, ties by ascending r + nIFFT (c - 1).  No cell: *n_left = 0,
 *                 and the call ends.
 *   4. pick       the first cell (r, c): row[i] = r, col[i] = c, hits[i], beam[i] = b* + 1, map_power[i] = M(r, c), rng[i] = (r - 1) rRes, beam_label[i] = beam_azi[b*], or
 *                 b* + 1 where beam_azi is NULL.
 *   5. refine     steps 1-3 of isac_refine.h on row r of R (the same device code, R as its row pointer; the periodogram sums all elements non-coherently): status[i], nu[i],
 *                 power[i] = P(nu*), the snapshot; vel[i] = nu* nFFT vRes (status 1: the grid velocity), on fft2D's axes.
 *      direction  azi[i] (and ele[i], UPA) = the lists' Bartlett scan of the snapshot (step 4 / 4' of the lists, the same device code).
 *                 status[i] == 1 (the row shows no maximum near the cell): parent[i] = i, the entry is recorded, nothing is subtracted, *n_left = the size of this pass's list,
 *                 and the call ends.
 *   6. parent     step 7 of isac_clean.h: parent[i] = the FIRST earlier kept entry k (parent[k] == k) with |r - row[k]| <= span_rows and |nu[i] - nu[k]| L <= merge_tol;
 *                 otherwise parent[i] = i (kept).  merge_tol == 0 disables the step.  A residue is still subtracted.
 *   7. cancel     step 8 of isac_clean.h, the same device code: for every window row r' with |r' - r| <= span_rows (clipped to the window's nr rows) and every element a, the
 *                 least-squares fit of the tone e^{+2 pi j nu l} over the active symbols is subtracted on those symbols.  The sum is that of isac_refine.h's X_a(nu): four
 *                 quarters of ceil(L / 4) in ascending l, joined (q0 + q1) + (q2 + q3); every phasor a sincos of the full argument ((-2 pi) nu) l, never a recurrence.
 * After max_iter entries one more run of steps 1-3 sets *n_left = the number of cells still listed (the count before the ISAC_MAX_TARGETS cut; 0: the map is exhausted).
 * *n_iter = the entries recorded (<= max_iter); *n_kept = those with parent[i] == i.  Of the last run of steps 1-3, whichever way the call ended: left_cells
 * [2 x ISAC_MAX_TARGETS] = the (row, col) pairs of its list in its order, the first min(*n_left, ISAC_MAX_TARGETS) of them; beam_pow [nr x nc x n_beams] = its planes.
 * snapshots [A x max_iter]: column i = the refined snapshot of entry i.  residual_rows [nr x L x A]: R after the last subtraction.  What lies behind *n_iter entries, or
 * behind the listed pairs, is not written.
 *
 * THE BAND UPDATE.  The definition recomputes the whole window in every pass; the library does not.  A subtraction changes the 2 span_rows + 1 rows of its band and nothing
 * else, so Pb, the per-CUT detector flags, M / b* and hits stay on the device across the passes, and after step 7 only the band's rows of Pb, the flags of the CUT rows
 * whose guard + training window meets the band, and M / b* / hits of those rows are formed again -- by the device functions the full pass runs, so every value is the one
 * a full recompute gives, bit for bit.  The local-maximum test and the list (O(nr nc)) are redone whole.
 *
 * sym_active, span_rows, merge_tol: isac_clean.h (defaults ISAC_CLEAN_SPAN_ROWS, ISAC_CLEAN_MERGE_TOL).
 *
 * ISAC_ERR_INVALID_ARG: W or m NULL; n_beams < 1; max_iter outside 1 .. ISAC_MAX_TARGETS; span_rows < 0; merge_tol negative or not finite; a NULL n_iter, n_kept, n_left,
 * row, col, hits, beam, status, parent, map_power, nu, vel, rng, power, azi or beam_label; no completed fft2D on the context, or a later call has rewritten its device state
 * (the cases of isac_fft2d_get_targets); a planar array without ele; a sym_active with no active symbol; a column of W with a zero or non-finite norm; a detector block
 * isac_fft2d_redetect refuses.  The arguments are checked first, the CPI second.
 * ISAC_ERR_UNSUPPORTED: n_beams > ISAC_MAX_BEAMS; nr nc n_beams >= 2^31; a halo (guard + training) of 0 in either dimension; the LDS refusal of
 * isac_fft2d_refine_targets; a UPA with more than 256 elements; more than 1024 elements; the detector limits of isac_fft2d_redetect; more than 4096 symbols.
 * On an error no output is written.  ULA and UPA alike.  Runs on the context's stream and returns when complete.  Off the timed path.
 *
 * OUT OF SCOPE: a MEX command; refinement on the beamformed series (step 5 sums the elements non-coherently: the benefit of a coherent sum at 64 or more elements is
 * unmeasured, and at 8 and 16 a NumPy prototype shows no difference); cancellation of spatial sidelobes within one cell (isac_resolve_directions on the returned snapshots
 * does that); deriving sym_active inside the library.
 */
#ifndef ISAC_BEAM_CLEAN_H
#define ISAC_BEAM_CLEAN_H

#include "isac.h"

#ifdef __cplusplus
extern "C" {
#endif

int isac_fft2d_beam_clean_targets(isac_ctx* ctx, const isac_c64* W /* host [A x n_beams] */, int32_t n_beams, const double* beam_azi /* [n_beams] labels, or NULL */,
                                  const isac_cfar_method* m, int32_t max_iter, int32_t span_rows, double merge_tol,
                                  const uint8_t* sym_active /* [L], 1 = transmitted; NULL = all */,
                                  int32_t* n_iter, int32_t* n_kept, int32_t* n_left,
                                  int32_t* row, int32_t* col, int32_t* hits, int32_t* beam, int32_t* status, int32_t* parent /* [max_iter] each */,
                                  double* map_power, double* nu, double* vel, double* rng, double* power, double* azi, double* ele, double* beam_label /* [max_iter] each; ele: required for a UPA, ignored (may be NULL) for a ULA */,
                                  isac_c64* snapshots /* [A x max_iter] or NULL */,
                                  isac_c64* residual_rows /* [nr x L x A] window rows after the last subtraction, or NULL */,
                                  double* beam_pow /* [nr x nc x n_beams] the planes of the last run of steps 1-3, or NULL */,
                                  int32_t* left_cells /* [2 x ISAC_MAX_TARGETS] the list of that run, or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* ISAC_BEAM_CLEAN_H */
