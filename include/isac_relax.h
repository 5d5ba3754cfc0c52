/*
 * isac_relax.h -- joint re-fit (RELAX) of Doppler tones on the last fft2D: an ADDITIVE part of the C ABI of libisac_hip.so under ISAC_ABI_VERSION 8 (one new entry point; no
 * new struct, no new isac_abi_sizeof selector; nothing that include/isac.h or the other additive headers declare changes).  Included by isac.h: include that.  Conventions: isac.h.
 *
 * isac_fft2d_clean_targets (isac_clean.h) extracts tones one after another: each frequency is estimated once, while every weaker tone of the same range rows is still in the
 * data, is subtracted and never looked at again.  Two tones that share a range row and lie one to three Doppler lobes apart (the unwindowed Doppler axis: -13 dB sidelobes)
 * bias each other's estimate, and the first subtraction leaves a residue.  The joint re-fit: with every other tone subtracted, put one tone back, estimate it again, subtract it
 * again -- tone after tone, cycle after cycle (Gauss-Seidel).  It removes the mutual bias, not the noise.  PROJECT-DEFINED.  Rows are 1-based.
 *
 * The call works on what the last completed fft2D left on the context (readiness and its errors: isac_fft2d_get_targets).  R is a copy of the window's range rows
 * ymid [nr x L x A] (natural symbol order) in scratch of the call's own; the rows themselves, the power window, the stored lists and every other getter's scratch stay
 * untouched.  The n entries (row[i], nu_in[i]) come from isac_fft2d_clean_targets, isac_fft2d_refine_targets or the caller; the call neither adds, drops nor merges one.
 * p_nu[l] = e^{-2 pi j nu l} on the active symbols and 0 on the inactive ones; every phasor is a sincos of the full argument ((-2 pi) nu) l, never a recurrence.  Every sum over
 * the symbols is that of isac_refine.h's X_a(nu): four quarters of ceil(L / 4), each quarter x += y p in ascending l from 0 (an inactive symbol enters with p = 0, so a NaN
 * there still spreads), joined (q0 + q1) + (q2 + q3).  C_i [span x A]: the amplitudes of tone i on the rows of its span, the window rows r' with |r' - row[i]| <= span_rows
 * (clipped to the window's nr rows).  fp64 throughout, no floating-point atomics.
 *   0. initialise  for i = 0 .. n - 1 in input order: nu_i = nu_in[i]; on every row r' of the span and every antenna a
 *                      C_i[r', a] = (sum_l R[r', l, a] p_{nu_i}[l]) / n_active,      R[r', l, a] -= C_i[r', a] conj(p_{nu_i}[l]) on the active symbols
 *                  -- step 8 of isac_clean.h, the same arithmetic.  cycles == 0: the call stops here, and R is the residual of isac_fft2d_clean_targets for the same
 *                  entries in the same order.
 *   1. cycles      for cycle = 1 .. cycles, for j = 0 .. n - 1 in input order:
 *      (a) centre  z[l, a] = R[row_j, l, a] + C_j[row_j, a] conj(p_{nu_j}[l]): the centre row with tone j restored, formed on the fly and never written back.
 *      (b) search  P_j(nu) = sum_a |X_a(nu)|^2, X_a(nu) = sum_l z[l, a] p_nu[l], and P_j' from the same sums (P' = (4 pi) sum_a Im(conj(X_a) D_a), D_a = sum_l l z p_nu,
 *                  summed over a ascending from 0.0): with h = box / L, if P_j'(nu_j - h) > 0 > P_j'(nu_j + h) the bracket [nu_j - h, nu_j + h] is halved 40 times on the
 *                  sign of P_j' at its midpoint (P' > 0: the lower end moves up) and nu_new is the midpoint of what is left.  Otherwise nu_new = nu_j: the entry stands, and
 *                  the cycle is marked for status.  A row that is all zero or holds a NaN never passes the test.  The 42 evaluations are made either way: the operation
 *                  count does not depend on the data.
 *      (c) re-fit  on every row r' of the span and every antenna a:
 *                      c_new = (sum_l (R[r', l, a] + C_j[r', a] conj(p_{nu_j}[l])) p_{nu_new}[l]) / n_active
 *                      R[r', l, a] = (R[r', l, a] + C_j[r', a] conj(p_{nu_j}[l])) - c_new conj(p_{nu_new}[l]) on the active symbols, one read-modify-write
 *                  then C_j[r', a] = c_new and nu_j = nu_new.
 *   2. outputs     nu[j] = nu_j; vel[j] = nu_j nFFT vRes, on fft2D's axes; s_a = n_active C_j[row_j, a]: power[j] = (sum_a |s_a|^2) / nFFT (ascending a from 0.0),
 *                  snapshots[:, j] = s / sqrt(nFFT) -- the periodogram and the snapshot of isac_refine.h of the restored tone; azi[j] (and ele[j], UPA) = the lists'
 *                  Bartlett scan of that snapshot (step 4 / 4' of the lists, the same device code); shift[j] = |nu_j - nu_in[j]| L; last_step[j] = |nu_new - nu_j| L of the
 *                  final cycle (cycles == 0: 0); status[j] = 0, or 1 if the test of (b) failed in the final cycle (cycles == 0: 0).  residual_rows [nr x L x A] = R
 *                  (nr = dims[0] of isac_fft2d_get_power_window).
 * SCHEDULE.  Entries whose spans share a row form, transitively, a cluster.  Clusters share no row, so they do not see each other.  The device runs the k-th entry (input
 * order) of every cluster side by side, k = 0, 1, ...: every row meets its entries in input order, and the result EQUALS that of the sequential sweep above, bit for bit.
 * Per (cycle, k) two launches and nothing read back until the end: the call costs (2 cycles + 1) x (the largest cluster) launch pairs.
 *
 * sym_active [L]: 1 = the symbol was transmitted; NULL = all (isac_clean.h).  box: the half width of the search in units of 1 / L; 0.5 keeps the search inside the main lobe
 * of the restored tone.  Convergence is geometric and slows as two tones approach: 1.3 / L apart 16 cycles reach 1e-13 / L, 0.8 / L apart about 4e-5 / L.
 *
 * ISAC_ERR_INVALID_ARG: n outside 0 .. ISAC_RELAX_MAX_TONES; with n > 0 a NULL row, nu_in, status, nu, vel, power, shift, last_step or azi; cycles outside 0 .. 64;
 * span_rows < 0; box not finite, <= 0 or > 2; a nu_in that is not finite; no completed fft2D on the context, or a later call has rewritten its device state (the cases of
 * isac_fft2d_get_targets); a planar array without ele; a row outside the CUT zone; a sym_active with no active symbol.  The arguments are checked first, the CPI second, and
 * all of it before any device work: a refused call writes nothing.  ISAC_ERR_UNSUPPORTED: the LDS refusal of isac_fft2d_refine_targets (the kernels here need less and
 * take its rule); a UPA with more than 256 elements.  n == 0 on a completed fft2D: ISAC_OK, and residual_rows (if given) is the copy of the range rows.
 * ULA and UPA alike.  Runs on the context's stream and returns when complete; a pending submit and its result buffer stay untouched.  Off the timed path.
 *
 * OUT OF SCOPE: a MEX command; deciding the number of tones; merging entries; off-grid range (the simulator delays an echo by whole samples: with nIFFT = Nfft true ranges
 * lie on the range grid); cancellation on beam planes; a range-sidelobe model beyond the row span; any change to the loop of isac_fft2d_clean_targets.
 */
#ifndef ISAC_RELAX_H
#define ISAC_RELAX_H

#include "isac.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISAC_RELAX_CYCLES 16            /* the defaults of sensing.estimation.relaxTargets; the span's is ISAC_CLEAN_SPAN_ROWS */
#define ISAC_RELAX_BOX 0.5
#define ISAC_RELAX_MAX_TONES 64

int isac_fft2d_relax_targets(isac_ctx* ctx, const int32_t* row /* [n] 1-based CUT rows */, const double* nu_in /* [n] cycles per symbol */, int32_t n,
                             int32_t cycles, int32_t span_rows, double box /* half width of the search in units of 1 / L */,
                             const uint8_t* sym_active /* [L], 1 = transmitted; NULL = all */,
                             int32_t* status, double* nu, double* vel, double* power, double* shift, double* last_step /* [n] each */,
                             double* azi, double* ele /* [n] each; ele: required for a UPA, ignored (may be NULL) for a ULA */,
                             isac_c64* snapshots /* [A x n] or NULL */,
                             isac_c64* residual_rows /* [nr x L x A] window rows after the last re-fit, or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* ISAC_RELAX_H */
