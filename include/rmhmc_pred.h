/*
 * rmhmc_pred.h — C-ABI of the posterior predictive probabilities in librmhmc_hip.so: given posterior draws in device memory, p(t* = 1 |
 * x*, data) of rows that were not in the training set, the spread of that probability over the draws, and the log pointwise predictive
 * density of held-out labels, computed where the draws are.  Same context and conventions as rmhmc.h.  Kept out of rmhmc.h: the CPU
 * oracle does not implement it.  Kernels: riemannhamiltonianmontecarlo_amd/csrc/pred.hip.h; host half: csrc/pred.h.  The specification
 * below is restated line by line in np.longdouble in tests/helpers/pred_ref.py.
 *
 * Inputs.  samples_dev [n][S][D] in device memory (what every *_sample_to call of rmhmc_out.h writes): the N = n S rows are the draws w_k.
 * xnew [R][D], host, every entry finite.  tnew [R], host, or NULL: every entry exactly 0.0 or 1.0.
 *
 * Invalid draws.  A draw with any non-finite entry is left out of every row, as in rmhmc_cov_partial_dev (a Gibbs chain that stopped has
 * NaN rows).  m is the number of draws used, the same for every row.  The device decides it in a pass of its own, before any product: an
 * infinite w_k times x can give a finite-looking p = 1.
 *
 * Per row r and used draw k.  f = x_r . w_k, e = exp(-|f|), hi = 1 / (1 + e), lo = e / (1 + e).  p = f >= 0 ? hi : lo, and the complement
 * 1 - p = f >= 0 ? lo : hi is never computed by subtraction, so both keep full relative accuracy down to the denormals.
 * q = tnew_r == 1 ? p : 1 - p is the likelihood of the held-out label under draw k.  An f that is NaN (the product met +inf and -inf)
 * makes the sums of that row NaN; m is unaffected.
 *
 * As in rmhmc_diag.h and rmhmc_adapt.h the work is split in two so that shards combine: a shard reduces its draws to a partial on its
 * device, and the partials are merged and finished on the host.  A partial of R rows is double[4 * R], rows of length R:
 *   row 0: m (an exact integer, in every entry)   row 1: S1 = sum over the used draws of p   row 2: S2 = sum of p^2
 *   row 3: SQ = sum of q; all zeros when tnew is NULL, written as -0.0, which no sum of likelihoods is: that is how the finish knows
 * Two partials merge by adding all four rows; one with m = 0 is the identity.  The sums are compensated (sum, error) pairs in a fixed
 * order that depends on (N, R, D) alone: no atomics, the same call on the same inputs gives the same bits, and different splits of the
 * draws agree to rounding.
 *
 * Finished.  prob_r = S1 / m.  pvar_r = max(0, S2 / m - prob_r^2), the population variance of p over the draws: all terms lie in [0, 1],
 * so the subtraction costs an absolute 4 * 2^-53 and no more.  lpd_r = log(SQ / m), the log pointwise predictive density, -inf when every
 * q underflowed; NaN without labels.  lpd_total = sum over r of lpd_r in row order.  m = 0 gives NaN everywhere.
 */
#ifndef RMHMC_PRED_H
#define RMHMC_PRED_H

#include "rmhmc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The partial of samples_dev [n][S][D] (device memory) for the rows xnew [R][D] and labels tnew [R] | NULL (host) -> partial_dev [4 * R]
 * (device memory).  Stream and synchronisation as rmhmc_ess_dev of rmhmc_out.h: the samples must be complete before the call, the
 * library's stream is idle on return.  The chain state and the training data of the context are not touched.  Checked on the host
 * before any device work, partial_dev untouched: RMHMC_ERR_INVALID for a NULL samples_dev, xnew or partial_dev, n < 1, S < 1, D < 1 or
 * R < 1, a non-finite entry of xnew, an entry of tnew other than 0 or 1; RMHMC_ERR_UNSUPPORTED for D > 256. */
int rmhmc_pred_partial_dev(rmhmc_ctx *ctx, const double *samples_dev, int64_t n, int64_t S, int32_t D, const double *xnew,
                           const double *tnew, int64_t R, double *partial_dev);

/* Host only, no context: merges the k partials (host pointers, all of the same R) in the order given and finishes.
 * merged [4 * R] (not one of the partials), prob [R], pvar [R], lpd [R], lpd_total [1], draws_used [1]: host, each may be NULL.
 * RMHMC_ERR_INVALID, nothing written, for k < 1, R < 1 or a NULL partial. */
int rmhmc_pred_finish(const double *const *partials, int32_t k, int64_t R, double *merged, double *prob, double *pvar, double *lpd,
                      double *lpd_total, int64_t *draws_used);

#ifdef __cplusplus
}
#endif

#endif /* RMHMC_PRED_H */
