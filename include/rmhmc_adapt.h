/*
 * rmhmc_adapt.h — C-ABI of the warm-up of the fixed-metric HMC sampler (rmhmc_phmc.h) in librmhmc_hip.so: the pooled mean and
 * covariance of many chains' samples, computed where the samples are; the regularised mass matrix made from it; dual averaging of
 * the step size; and the windowed warm-up that puts them together.  Same context and conventions as rmhmc.h.  Kept out of rmhmc.h:
 * the CPU oracle does not implement it.  Kernels: riemannhamiltonianmontecarlo_amd/csrc/adapt.hip.h; host half: csrc/adapt.h.
 *
 * Pooled covariance.  samples [n][S][P] (what every *_sample_to call of rmhmc_out.h writes, P = D): the N = n S rows are pooled.  A
 * row with any non-finite entry is left out entirely (a Gibbs chain that stopped has NaN rows).  As in rmhmc_diag.h the work is split
 * in two so that shards combine: a shard reduces its samples to a partial on its device, and the partials are merged and finished on
 * the host.  A partial of P is double[(2 + P) * P], rows of length P:
 *   row 0: m, the rows used (an exact integer, in every entry)   row 1: the mean of the used rows
 *   row 2 + i: row i of C = sum over the used rows of (x - mean)(x - mean)', full and exactly symmetric
 * The device centres the rows about the mean it has summed (two passes; never E[xx'] - mean mean').  Two partials merge by Chan's
 * update (delta = mean_b - mean_a, mean = mean_a + delta m_b / m, C = C_a + C_b + delta delta' m_a m_b / m); one with m = 0 is the
 * identity.  cov = C / (m - 1), NaN for m < 2.  The same call on the same samples gives the same bits (no atomics, fixed summation
 * order); different splits of the rows agree to rounding, not to the bit.  Row 1 is a double: a merge sees the means of its
 * partials rounded to |mean| 2^-53, so the merged C carries an error of up to 2 |delta_i| |mean_j| 2^-53 m_a m_b / m per entry on top of
 * the rounding of the sums - negligible unless |mean| is many orders of magnitude above the spread.
 *
 * Regularised mass.  Sigma_reg = m / (m + 5) cov + 1e-3 * 5 / (m + 5) I (the shrinkage of Stan's warm-up), Mass = Sigma_reg^-1.
 *
 * Dual averaging of log eps (Hoffman & Gelman 2014, section 3.2), one update per window of acceptance statistic a.  The state is
 * double[4] = (t, Hbar, log epsbar, mu):
 *   t += 1;  Hbar = (1 - 1 / (t + t0)) Hbar + (delta - a) / (t + t0);  log eps = mu - sqrt(t) / gamma Hbar;
 *   log epsbar = t^-kappa log eps + (1 - t^-kappa) log epsbar;   eps_next = exp(log eps), eps_bar = exp(log epsbar)
 * A (re)start at eps is t = 0, Hbar = 0, log epsbar = 0, mu = log(factor eps): the iterates shrink towards factor eps.  The paper's
 * factor is 10, chosen for hundreds of cheap updates; the warm-up below starts with it and restarts with factor 1 after a mass
 * update.  (With one update per window and a mass update in most windows a restart at 10 eps is never recovered from: a single
 * update takes eps down by e^-1.45 at most, so eps grows 2.3-fold per window - measured on the pima data, 64 chains, 12 windows of
 * 25: eps = 3500 and no accepted proposal on each of 8 seeds, against an acceptance of 0.78 to 0.82 with factor 1.)
 */
#ifndef RMHMC_ADAPT_H
#define RMHMC_ADAPT_H

#include "rmhmc_phmc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The partial of samples_dev [n][S][P] (device memory) -> partial_dev [(2 + P) * P] (device memory).  Stream and synchronisation as
 * rmhmc_ess_dev of rmhmc_out.h: the samples must be complete before the call, the library's stream is idle on return.  The chain state
 * of the context is not touched.  RMHMC_ERR_INVALID for a NULL pointer, n < 1, S < 1 or P < 1; RMHMC_ERR_UNSUPPORTED for P > 256. */
int rmhmc_cov_partial_dev(rmhmc_ctx *ctx, const double *samples_dev, int64_t n, int64_t S, int32_t P, double *partial_dev);

/* Host only, no context: merges the k partials (host pointers, all of the same P) in the order given and finishes.
 * merged [(2 + P) * P] (not one of the partials), mean [P], cov [P * P], rows_used [1]: host, each may be NULL.
 * RMHMC_ERR_INVALID for k < 1, P < 1 or a NULL partial. */
int rmhmc_cov_finish(const double *const *partials, int32_t k, int32_t P, double *merged, double *mean, double *cov,
                     int64_t *rows_used);

/* Host only: mass_out [P * P] = Sigma_reg^-1 from cov [P * P] of m rows.  RMHMC_ERR_INVALID, mass_out untouched, for a NULL pointer,
 * P < 1, m < 2, or a Sigma_reg that is not finite or not positive definite (the caller keeps its previous mass). */
int rmhmc_adapt_mass(const double *cov, int64_t m, int32_t P, double *mass_out);

/* Host only: the (re)start of the dual-averaging state at step size eps, mu = log(factor eps).  RMHMC_ERR_INVALID unless eps and
 * factor are finite and > 0. */
int rmhmc_adapt_init(double state[4], double eps, double factor);

/* Host only: one dual-averaging update with the acceptance statistic `accept` of a window; delta the target (0.8), gamma (0.05),
 * t0 (10), kappa (0.75).  eps_next: the step size of the next window; eps_bar: the averaged one, the result of a warm-up that ends
 * here; either may be NULL.  RMHMC_ERR_INVALID, state untouched, for a non-finite accept or a step size that is not finite and > 0. */
int rmhmc_adapt_step(double state[4], double accept, double delta, double gamma, double t0, double kappa, double *eps_next,
                     double *eps_bar);

/* The warm-up of rmhmc_phmc_sample_to; dual averaging starts at eps0 with factor 10.  The context has its data and a mass (rmhmc_phmc_set_mass; the identity is allowed).
 * theta0 [n][D] | NULL: zeros.  Schedule: W windows, window w of win_len[w] >= 1 iterations and kind win_kind[w]: 0 adapts the step
 * size, 1 the step size and then the mass.  Window w runs win_len[w] iterations of rmhmc_phmc_sample_to's body with burn_in = 0, the
 * current mass and step size, seed + 1 + w (mod 2^64) and chain_offset, from the last positions of window w - 1, into a device buffer
 * of the call's own; then a = (sum over the chains of their accepted proposals) / (n win_len[w]) goes through rmhmc_adapt_step.  In
 * a window of kind 1 the window's covariance partial is then merged into a running partial; once that holds >= min_rows rows,
 * rmhmc_adapt_mass is tried on it: on success the mass is installed with rmhmc_phmc_set_mass, the running partial is emptied and the
 * dual averaging restarts at the step size of the next window with factor 1; on refusal the previous mass stays, the running partial is kept
 * and the warm-up goes on.
 * Outputs (host, each may be NULL): eps_out: eps_bar of the last window; mass_out [D * D]: the last mass installed (all NaN when none
 * was: the context's mass is the caller's); theta_out [n][D]: the last positions; eps_trace [W]: the step size each window ran with;
 * accept_trace [W]: its a; mass_updated [W]: 1 installed, -1 tried and refused, 0 not tried; seconds_out: host wall time of the call.
 * The context is left with the final mass; like every sampling call it invalidates the chain state.  The call equals the composition
 * of the public pieces run by the caller with the same seeds, bit for bit.
 * RMHMC_ERR_INVALID: a NULL schedule, W < 1, a window shorter than 1 or of a kind other than 0 / 1, L < 1, min_rows < 1, eps0 not
 * finite and > 0, no mass set; RMHMC_ERR_UNSUPPORTED: D > 256. */
int rmhmc_phmc_warmup(rmhmc_ctx *ctx, const double *theta0, int32_t L, double eps0, double delta, double gamma, double t0,
                      double kappa, uint64_t seed, int64_t chain_offset, int32_t W, const int64_t *win_len, const int32_t *win_kind,
                      int64_t min_rows, double *eps_out, double *mass_out, double *theta_out, double *eps_trace,
                      double *accept_trace, int32_t *mass_updated, double *seconds_out);

#ifdef __cplusplus
}
#endif

#endif /* RMHMC_ADAPT_H */
