/*
 * rmhmc_diag.h — C-ABI of the cross-chain diagnostics of librmhmc_hip.so: split R-hat and the pooled effective sample size of
 * many chains, computed where the samples are.  Same context and conventions as rmhmc.h.  Kept out of rmhmc.h: the CPU oracle does
 * not implement it.
 *
 * samples [n][S][P] (what every *_sample_to call of rmhmc_out.h writes, P = D).  H = S / 2; every chain gives two series per
 * dimension, its first H rows and its last H rows (odd S: the middle row is unused).  A series with a non-finite value is left out
 * of its dimension only; a Gibbs chain that stopped has NaN rows and so drops out of every dimension.  Per used series j: its mean,
 * the biased autocovariances acov_j(t) = (1/H) sum_{s=0}^{H-1-t} (x_s - mean_j)(x_{s+t} - mean_j) of the centred series for
 * t = 0 .. T-1, and s2_j = acov_j(0) H / (H - 1).  Pooled over the m series used in a dimension:
 *   W = (sum_j s2_j) / m,  B/H = M2 / (m - 1) with M2 = sum_j (mean_j - mean of the means)^2,  var+ = W (H-1)/H + B/H,
 *   rhat = sqrt(var+ / W),
 *   rho_0 = 1, rho_t = 1 - (W - (sum_j acov_j(t)) / m) / var+,  Gamma_k = rho_2k + rho_2k+1, each replaced by the running minimum,
 *   summed while Gamma_k > 0 and 2k+1 < T (the rule of the per-chain ESS),  tau = max(1, -1 + 2 sum),  ess = m H / tau,
 *   pairs = number of Gamma_k summed.  2 pairs + 1 >= T: the lags ran out before the sequence ended and ess is an upper bound; this
 *   is always so when the chains disagree (rho_t then tends to 1 - W / var+ > 0).  m < 2, or W not > 0: rhat = ess = NaN, pairs = 0.
 *
 * The work is split in two so that shards combine: every shard reduces its samples to a partial on its device, and the partials, a
 * few KB each, are merged and finished on the host.  A partial of (H, T, P) is double[(4 + T) * P], rows of length P:
 *   row 0: m (exact integers)   row 1: the mean of the used series' means   row 2: M2   row 3: sum_j s2_j
 *   row 4 + t: sum_j acov_j(t), t = 0 .. T-1
 * Two partials merge by adding rows 0, 3 and 4.., and by Chan's update of rows 1 and 2 (delta = mean_b - mean_a,
 * mean = mean_a + delta m_b / m, M2 = M2_a + M2_b + delta^2 m_a m_b / m); one with m = 0 is the identity.  The same call on the same
 * samples gives the same bits; different splits of the chains agree to rounding, not to the bit.
 */
#ifndef RMHMC_DIAG_H
#define RMHMC_DIAG_H

#include "rmhmc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The partial of samples_dev [n][S][P] (device memory) -> partial_dev [(4 + T) * P] (device memory), T = max_lag + 1;
 * max_lag = 0 means H - 1 (every lag).  Stream and synchronisation as rmhmc_ess_dev (rmhmc_out.h): the samples must be complete
 * before the call, the library's stream is idle on return.  The chain state of the context is not touched.
 * RMHMC_ERR_UNSUPPORTED unless 4 <= S <= 20000 (the centred series is held in LDS); RMHMC_ERR_INVALID for a NULL pointer, n < 1,
 * P < 1 or max_lag outside 0 .. H-1. */
int rmhmc_diag_partial_dev(rmhmc_ctx *ctx, const double *samples_dev, int64_t n, int64_t S, int32_t P, int64_t max_lag,
                           double *partial_dev);

/* Host only, no context: merges the k partials (host pointers, all of the same (H, T, P)) in the order given and finishes.
 * merged [(4 + T) * P] (not one of the partials), rhat, ess, pairs, chains_used [P] each: host, each may be NULL; chains_used is row 0.
 * RMHMC_ERR_INVALID for k < 1, H < 2, T outside 2 .. H, P < 1 or a NULL partial. */
int rmhmc_diag_finish(const double *const *partials, int32_t k, int64_t H, int64_t T, int32_t P, double *merged, double *rhat,
                      double *ess, int64_t *pairs, int64_t *chains_used);

#ifdef __cplusplus
}
#endif

#endif /* RMHMC_DIAG_H */
