/*
 * isac_clean.h -- successive target cancellation (CLEAN) on the last fft2D: an ADDITIVE part of the C ABI of libisac_hip.so under ISAC_ABI_VERSION 8 (one new entry point; no
 * new struct, no new isac_abi_sizeof selector; nothing that include/isac.h or the other additive headers declare changes).  Included by isac.h: include that.  Conventions: isac.h.
 *
 * The lists (isac_fft2d_get_targets, isac_fft2d_get_targets_upa, isac_fft2d_beam_detect) and isac_fft2d_refine_targets read ONE range-Doppler map of the CPI.  On that map a
 * strong echo's unwindowed Doppler response (-13 dB Dirichlet sidelobes, the split lobes of the symbol half swap, the gap lobes of a silent 'S' slot) is listed as extra
 * entries, and a weaker echo in the same or a neighbouring range row is hidden under those sidelobes and under the CFAR threshold they raise: it is no local maximum of the
 * map and its cell fails the detector, so no list, beam or refinement returns it.  Successive cancellation: take the strongest detection, estimate its tone off the grid,
 * subtract that tone from the range rows, detect again on what is left.  PROJECT-DEFINED.  Indices are 1-based; parent[] holds 0-based entry indices.
 *
 * The call works on what the last completed fft2D left on the context (readiness and its errors: isac_fft2d_get_targets).  R is a copy of the window's range rows
 * ymid [nr x L x A] (natural symbol order) in scratch of the call's own; the rows themselves, the power window, the stored lists and every other getter's scratch stay
 * untouched.  For pass i = 0, 1, ...:
 *   1. planes     P[r, c, a] = |rdm(r, c, a)|^2 on every cell of the power window, rdm(r, c, a) formed from R by the chain of isac_fft2d_get_rdm_window (the single-bin DFT
 *                 over the symbols after the half swap, four quarters joined (q0 + q1) + (q2 + q3), / sqrt(nFFT)); the modulus is two rounded products and one rounded sum,
 *                 never contracted.  (Pass 0 therefore differs from the CPI's own power window by that chain's rounding against the Doppler FFT's.)
 *   2. detect     detector m with the stored isac_cfar_config (CUT zone, guard / training bands, pfa) on every antenna plane: the device code of isac_fft2d_redetect.
 *   3. cells      steps 1, 2 and 5 of isac_fft2d_get_targets on P and those lists: S = sum_a P (ascending a from 0.0), hits >= 1, S strictly above all 8 neighbours, order
 *                 by S descending (ties: ascending column-major index).  No cell: *n_left = 0, and the call ends.
 *   4. pick       the first cell (r, c): row[i] = r, col[i] = c, hits[i], map_power[i] = S(r, c), rng[i] = (r - 1) rRes.
 *   5. refine     steps 1-3 of isac_refine.h on row r of R (the same device code, R as its row pointer): status[i], nu[i], power[i] = P(nu*), the snapshot; vel[i] = nu* nFFT
 *                 vRes (status 1: the grid velocity), on fft2D's axes.
 *   6. direction  azi[i] (and ele[i], UPA) = the lists' Bartlett scan of the snapshot (step 4 / 4' of the lists, the same device code).
 *                 status[i] == 1 (the row shows no maximum near the cell): parent[i] = i, the entry is recorded, nothing is subtracted, *n_left = the size of this pass's list,
 *                 and the call ends.
 *   7. parent     parent[i] = the FIRST earlier kept entry k (parent[k] == k) with |r - row[k]| <= span_rows and |nu[i] - nu[k]| L <= merge_tol: entry i is a residue of an
 *                 imperfect subtraction.  Otherwise parent[i] = i (kept).  merge_tol == 0 disables the step.  A residue is still subtracted.
 *   8. cancel     for every window row r' with |r' - r| <= span_rows (clipped to the window's nr rows) and every antenna a:
 *                     c = (sum_{l active} y[r', l, a] e^{-2 pi j nu l}) / n_active,      y[r', l, a] -= c e^{+2 pi j nu l} on the active symbols only
 *                 -- the least-squares fit of the tone over the transmitted symbols.  fp64 throughout.  The sum is that of isac_refine.h's X_a(nu): the L symbols in four quarters
 *                 of ceil(L / 4), each quarter x += y p in ascending l from 0 (an inactive symbol enters with p = 0, so a NaN there still spreads), joined (q0 + q1) + (q2 + q3);
 *                 every phasor is a sincos of the full argument ((-2 pi) nu) l, never a recurrence; c = (Re X / n_active, Im X / n_active); y - c conj(p).
 * After max_iter entries one more run of steps 1-3 sets *n_left = the number of cells still listed (the count before the ISAC_MAX_TARGETS cut; 0: the map is exhausted).
 * *n_iter = the entries recorded (<= max_iter); *n_kept = those with parent[i] == i.  snapshots [A x max_iter]: column i = the refined snapshot of entry i.  residual_rows
 * [nr x L x A]: R after the last subtraction (nr = dims[0] of isac_fft2d_get_power_window).
 *
 * sym_active [L]: 1 = the symbol was transmitted; NULL = all.  A tone fitted across a silent slot (zeroed rows) is under-estimated by n_active / L and its residue masks what
 * the pass was meant to uncover: the caller, who knows the slot format, names the silent symbols.
 * span_rows: the Kaiser range window spreads an echo over the neighbouring rows; with 0 the rows +-1 still mask a weak target of the same range, with 1 the strong target's
 * residues two rows away are listed.  Default 2.
 *
 * ISAC_ERR_INVALID_ARG: m NULL; max_iter outside 1 .. ISAC_MAX_TARGETS; span_rows < 0; merge_tol negative or not finite; a sym_active with no active symbol; a NULL n_iter,
 * n_kept, n_left, row, col, hits, status, parent, map_power, nu, vel, rng, power or azi; a planar array without ele; no completed fft2D on the context, or a later call has
 * rewritten its device state (the cases of isac_fft2d_get_targets); a detector block isac_fft2d_redetect refuses.  The arguments are checked first, the CPI second.
 * ISAC_ERR_UNSUPPORTED: a halo (guard + training) of 0 in either dimension; the LDS refusal of isac_fft2d_refine_targets; a UPA with more than 256 elements.
 * ULA and UPA alike.  Runs on the context's stream and returns when complete; a pending submit and its result buffer stay untouched.  Off the timed path: every pass
 * recomputes the whole window.
 *
 * A joint re-fit of all extracted tones (RELAX) is a call of its own on this call's entries: isac_fft2d_relax_targets (isac_relax.h).
 * OUT OF SCOPE: a MEX command; deriving sym_active inside the library; cancellation on beam planes; a range-sidelobe model beyond the row span.
 */
#ifndef ISAC_CLEAN_H
#define ISAC_CLEAN_H

#include "isac.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISAC_CLEAN_SPAN_ROWS 2          /* the defaults of sensing.estimation.cleanTargets */
#define ISAC_CLEAN_MERGE_TOL 0.5

int isac_fft2d_clean_targets(isac_ctx* ctx, const isac_cfar_method* m, int32_t max_iter, int32_t span_rows, double merge_tol,
                             const uint8_t* sym_active /* [L], 1 = transmitted; NULL = all */,
                             int32_t* n_iter, int32_t* n_kept, int32_t* n_left,
                             int32_t* row, int32_t* col, int32_t* hits, int32_t* status, int32_t* parent /* [max_iter] each */,
                             double* map_power, double* nu, double* vel, double* rng, double* power, double* azi, double* ele /* [max_iter] each; ele: required for a UPA, ignored (may be NULL) for a ULA */,
                             isac_c64* snapshots /* [A x max_iter] or NULL */,
                             isac_c64* residual_rows /* [nr x L x A] window rows after the last subtraction, or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* ISAC_CLEAN_H */
