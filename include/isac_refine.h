/*
 * isac_refine.h -- refinement of a target list of the last fft2D: an ADDITIVE part of the C ABI of libisac_hip.so under ISAC_ABI_VERSION 8 (one new entry point; no new
 * struct, no new isac_abi_sizeof selector; nothing that include/isac.h or the other additive headers declare changes).  Included by isac.h: include that.  Conventions: isac.h.
 *
 * The lists (isac_fft2d_get_targets, isac_fft2d_get_targets_upa, isac_fft2d_beam_detect) read a target off the range-Doppler grid: the velocity is quantised to a Doppler
 * bin, and -- fft2D.m:44 swaps the two halves of the symbol axis before the Doppler FFT -- a tone whose phase does not advance by a whole number of turns over the L symbols
 * shows a SPLIT Doppler peak, so one target is listed several times, next to its Doppler sidelobes.  The range rows of the last fft2D stay on the device in natural symbol
 * order, without the swap: the exact off-grid periodogram of every listed cell is available.  PROJECT-DEFINED.  Indices are 1-based; the indices in
 * parent[] and sidelobe_of[] are 0-based INPUT indices.
 *
 * For entry i: r its range row, k = col - nFFT/2 - 1, y[l,a] the L symbols of range row r, antenna a, in natural order (no half swap, no truncation: all L symbols, also
 * where nFFT < L),  X_a(nu) = sum_{l=0}^{L-1} y[l,a] e^{-2 pi j nu l},  P(nu) = sum_a |X_a(nu)|^2 / nFFT (antenna sum in ascending order, fp64).
 *   1. probes      nu0 = k / nFFT, W = max(1/L, 1/nFFT), M = ceil(8 L W), nu_g = nu0 + g W / M for g = -M .. M.  With nFFT >= L: 17 probes over +-1/L; a split lobe sits
 *                  about +-0.6/L from its tone, so either lobe's window holds the true peak.
 *   2. peak        interior probes with P_g > P_{g-1} and P_g >= P_{g+1} are local maxima; the one with the largest P is taken, on a tie the lowest g.  None (an all-zero
 *                  or NaN row): status = 1, nu = nu0, vel = the grid velocity, power = P(nu0), snapshot = X(nu0) / sqrt(nFFT), parent = i, and steps 3-5 skip the entry.
 *                  Otherwise status = 0.
 *   3. maximiser   nu* = the zero of P'(nu) in [nu_{g-1}, nu_{g+1}], P' = (2/nFFT) sum_a Re(conj(X_a) X_a'), X_a' = sum_l -2 pi j l y e^{-2 pi j nu l}; the library bisects on
 *                  the sign of P' (40 halvings of the bracket 2 W / M, which leave 2.3e-13 / L of it where nFFT >= L; every entry the same count).  nu = nu*; vel = nu* nFFT vRes (fft2D's own velocity axis: it
 *                  inherits whatever scale that axis has); power = P(nu*); snapshot x[a] = X_a(nu*) / sqrt(nFFT); azi (and ele, UPA) = the first arg-max of the Bartlett
 *                  scan of isac_fft2d_get_targets (step 4) / isac_fft2d_get_targets_upa (step 4') on x -- the same device code over the same grids.
 *   4. merge       (host, in input order)  entry i with status 0 is absorbed by the FIRST earlier kept entry k with status 0, |row_i - row_k| <= merge_rows and
 *                  |nu_i - nu_k| L <= merge_tol: parent[i] = k.  Otherwise parent[i] = i (kept).  Input order, not refined power, on purpose: two lobes of one tone
 *                  converge to the same maximum and their powers differ only by rounding.
 *   5. sidelobes   (host)  for each kept entry i with status 0: sidelobe_of[i] = the lowest-index kept k != i with status 0, |row_i - row_k| <= merge_rows, P_k > P_i and
 *                  P_i <= sidelobe_margin P_k D^2(nu_i - nu_k), D(d) = sin(pi d L) / (L sin(pi d)), D(0) = 1 -- the Doppler response of an unwindowed L-symbol tone.
 *                  -1 when there is none, and for every entry that is not kept or has status 1.  Entries are flagged, never removed: the caller filters.
 * *n_kept = the number of i with parent[i] == i.  The values of an absorbed entry (nu, vel, power, azi, ele, snapshot) are its own.
 *
 * ISAC_ERR_INVALID_ARG: n < 0 or n > ISAC_MAX_TARGETS; n_kept NULL; with n > 0 a NULL row, col, status, parent, sidelobe_of, nu, vel, power or azi, or -- a planar
 * array -- a NULL ele; merge_tol or sidelobe_margin negative or not finite; merge_rows < 0; no completed fft2D on the context, or -- rather than a stale answer -- a later
 * call has rewritten its device state (the cases of isac_fft2d_get_targets); a (row, col) outside the CUT zone of that CPI.  The arguments are checked first, the CPI second:
 * n == 0 on a context with a completed fft2D returns ISAC_OK with *n_kept = 0.  merge_tol == 0 disables step 4 (every entry is kept: the two lobes of one tone can reach
 * the very same nu* bit for bit, and "no tolerance" must not hinge on that); sidelobe_margin == 0 disables step 5; a halo of 0 is fine (no neighbour test is made).
 * ISAC_ERR_UNSUPPORTED: (2M + 2) L + 2 A complex values do not fit the 160 KB of LDS of a compute unit (about 560 symbols with nFFT >= L); a UPA with more than 256 elements.
 * ULA and UPA alike, the UPA with ISAC_OPT_UPA_DOA on or off.  Runs on the context's stream in scratch of its own and returns when complete; every other getter's answer, a
 * pending submit and its result buffer stay untouched.
 *
 * OUT OF SCOPE: off-grid range (only a window of range rows is kept: band-limited interpolation would be approximate -- a call of its own on the two grids:
 * isac_range_refine_dev, isac_subsample.h); off-grid direction (a call of its own on the snapshots this one returns: isac_resolve_directions, isac_directions.h); merging of range sidelobes (the
 * Kaiser range window leaves none in the project's scenes); a MEX command.
 */
#ifndef ISAC_REFINE_H
#define ISAC_REFINE_H

#include "isac.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ISAC_REFINE_MERGE_TOL 0.5       /* the defaults of sensing.estimation.refineTargets */
#define ISAC_REFINE_MERGE_ROWS 1
#define ISAC_REFINE_SIDELOBE_MARGIN 2.0

int isac_fft2d_refine_targets(isac_ctx* ctx, const int32_t* row, const int32_t* col, int32_t n /* 1-based rdm cells, e.g. a list's row[] / col[] */,
                              double merge_tol, int32_t merge_rows, double sidelobe_margin,
                              int32_t* n_kept,
                              int32_t* status, int32_t* parent, int32_t* sidelobe_of /* [n] each, INPUT indices */,
                              double* nu, double* vel, double* power, double* azi, double* ele /* [n] each; ele: required for a UPA, ignored (may be NULL) for a ULA */,
                              isac_c64* snapshots /* [A x n] or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* ISAC_REFINE_H */
