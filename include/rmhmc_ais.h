/*
 * rmhmc_ais.h — C-ABI of the log marginal likelihood log p(t) = log of the integral of p(t|w) p(w) dw by annealed importance sampling
 * (AIS, Neal 2001) in librmhmc_hip.so: the fixed-metric HMC sampler of rmhmc_phmc.h on tempered targets, exact draws from the prior,
 * the reduction of the importance weights, and the run that puts them together.  Same context and conventions as rmhmc.h (host
 * buffers unless a name ends in _dev, float64, chain-major, int status, rmhmc_last_error).  Kept out of rmhmc.h: the CPU oracle does not
 * implement it.  Kernels: riemannhamiltonianmontecarlo_amd/csrc/ais.hip.h; host half: csrc/ais.h.
 *
 * Tempered target.  LJL_beta(w) = beta loglik(w) + logprior(w), beta finite and >= 0:
 *   loglik(w)   = sum_n t_n f_n - log(1 + exp f_n), f = X w: the likelihood part of LJL, the naive log(1 + exp f) included
 *   logprior(w) = -D/2 log(2 pi alpha) - w'w / (2 alpha): the Gaussian term with its constant
 *   grad_beta   = beta grad_lik - w / alpha, grad_lik = X'(t - p)
 * A tempered transition is the transition of rmhmc_phmc.h with LJL_beta and grad_beta in place of LJL and grad: the same streams,
 * trajectory length, NaN rule, failure rule (RMHMC_ST_NONFINITE) and acceptance.  At beta = 0 a chain whose loglik is not finite has
 * LJL_0 = 0 * inf = NaN: it fails, as it does at every other beta.
 * At a position with an entry that is not finite some row has t f = 0 * inf or f - log(1 + exp f) = inf - inf: loglik is NaN there.
 *
 * Two equalities anchor the tempered sampler to tested code:
 *   beta = 1           rmhmc_tphmc_transition and rmhmc_tphmc_sample_to equal rmhmc_phmc_transition and rmhmc_phmc_sample_to bit for bit
 *                      in every common output (1 x is exact; the sums keep their order)
 *   a ladder of ones   rmhmc_ais_run with a theta0, beta0 = 1, every beta[k] = 1 and stage_mass NULL: logw is exactly 0 for every chain
 *                      whose loglik is finite, and the positions after stage k are those of the corresponding rmhmc_phmc_sample_to calls
 *
 * Importance weights.  logw[n]: -inf is a legitimate weight of zero and counts; NaN marks a chain that failed and is left out.  As in
 * rmhmc_adapt.h the reduction is split so that shards combine: a partial is double[5] =
 *   (m: entries used, n_nan: entries left out, a: the maximum of the used entries, S1 = sum exp(lw - a), S2 = sum exp(2 (lw - a)))
 * over the used entries; if every used entry is -inf (or m = 0) then a = -inf and S1 = S2 = 0.  Two partials merge by a = max(a_1, a_2),
 * S_i = S_i1 exp(i (a_1 - a)) + S_i2 exp(i (a_2 - a)), m and n_nan added; a partial with m = 0 is the identity (its n_nan is still
 * counted).  Finished:
 *   log_mean_w = a + log(S1 / m)     se = sqrt((m S2 / S1^2 - 1) / (m - 1)), the delta-method standard error of log_mean_w, NaN for m < 2
 *   weight_ess = S1^2 / S2
 * The same call on the same logw gives the same bits (no atomics; the order of every sum depends on n alone); different splits agree to
 * rounding.  Rounding bound of S1 and S2 against exact arithmetic: a term exp(x), x = lw - a <= 0, with x < -745.2 is 0 in a double and
 * below 5e-324 exactly; otherwise the subtraction leaves |x| 2^-53 <= 746 * 2^-53 in the exponent, which is the relative error of the
 * term, and exp adds 1 ulp.  The terms are positive and the sums compensated (sum, error) pairs, so S1 and S2 are good to
 * 748 * 2^-53 = 8.3e-14 relative for any n and any spread of logw; a merge adds as much again; a, m and n_nan are exact.
 */
#ifndef RMHMC_AIS_H
#define RMHMC_AIS_H

#include "rmhmc_phmc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The iteration counter of the prior draws: rmhmc_ais_prior takes its normals from the library's stream of momentum normals (blocks
 * d / 2 of key (seed, chain_offset + c)) at this counter.  A sampler reaches it only in a run of 2^32 transitions of one call. */
#define RMHMC_AIS_PRIOR_ITER 0xFFFFFFFFu

/* One tempered transition with caller-supplied randomness: arguments as rmhmc_phmc_transition, then beta, loglik0_out [n] | NULL: loglik
 * at the start positions, loglik_out [n] | NULL: loglik at the returned w.  H_cur_out and H_prop_out are those of LJL_beta.
 * RMHMC_ERR_INVALID as rmhmc_phmc_transition, no mass set included, and for a beta that is not finite or < 0. */
int rmhmc_tphmc_transition(rmhmc_ctx *ctx, double *w, const double *z, const double *u_len, const double *u_acc, int32_t L, double eps,
                           int32_t *accepted_out, int32_t *nsteps_out, double *H_cur_out, double *H_prop_out, double *w_prop_out,
                           double *p_prop_out, int32_t *status_out, double beta, double *loglik0_out, double *loglik_out);

/* The power-posterior sampler at one beta, every output mode of rmhmc_out.h: arguments and contract as rmhmc_phmc_sample_to, then
 * beta, loglik0_out [n] | NULL: loglik of the initial evaluation at theta0, loglik_out [n] | NULL: loglik at the last state; both host
 * pointers whatever the descriptor says.  RMHMC_ERR_INVALID also for a beta that is not finite or < 0. */
int rmhmc_tphmc_sample_to(rmhmc_ctx *ctx, int64_t n_iter, int64_t burn_in, int32_t L, double eps, uint64_t seed, int64_t chain_offset,
                          const double *theta0, const rmhmc_out *out, int64_t *accept_out, int64_t *steps_out, double *seconds_out,
                          double beta, double *loglik0_out, double *loglik_out);

/* Exact draws from the prior: theta_out [n][D], w = sqrt(alpha) z, z the normals of key (seed, chain_offset + c) at iteration counter
 * RMHMC_AIS_PRIOR_ITER.  The chain state of the context is not touched.  RMHMC_ERR_INVALID for a NULL pointer. */
int rmhmc_ais_prior(rmhmc_ctx *ctx, uint64_t seed, int64_t chain_offset, double *theta_out);

/* The partial of logw_dev [n] (device memory) -> partial_dev [5] (device memory).  Stream and synchronisation as rmhmc_ess_dev of
 * rmhmc_out.h; the chain state is not touched.  RMHMC_ERR_INVALID for a NULL pointer or n < 1. */
int rmhmc_ais_partial_dev(rmhmc_ctx *ctx, const double *logw_dev, int64_t n, double *partial_dev);

/* Host only, no context: merges the k partials (host pointers) in the order given and finishes.  merged [5] | NULL, log_mean_w | NULL,
 * se | NULL, weight_ess | NULL, m_out | NULL, n_nan_out | NULL.  With m = 0 log_mean_w, se and weight_ess are NaN; with S1 = 0
 * log_mean_w is -inf and se and weight_ess are NaN.  RMHMC_ERR_INVALID for k < 1 or a NULL partial. */
int rmhmc_ais_finish(const double *const *partials, int32_t k, double *merged, double *log_mean_w, double *se, double *weight_ess,
                     int64_t *m_out, int64_t *n_nan_out);

/* The annealing run.  The context has its data and a mass (rmhmc_phmc_set_mass; the identity is allowed).  theta0 [n][D] | NULL: the run
 * starts from rmhmc_ais_prior(seed, chain_offset), which requires beta0 = 0.  logw starts at 0.  Stage k = 0 .. T - 1:
 *   if stage_mass and stage_mass[k]: Mass = beta[k] H_lik + I / alpha is installed through the path of rmhmc_phmc_set_mass; a refusal
 *     keeps the previous mass and the run goes on
 *   stage_len[k] iterations of rmhmc_tphmc_sample_to's body at beta[k] with burn_in = 0, seed + 1 + k (mod 2^64) and chain_offset, from
 *     the last positions of stage k - 1 (theta0, or the prior draws, for k = 0)
 *   logw += (beta[k] - beta[k - 1]) loglik0 of this stage, beta[-1] = beta0 (a product and a sum, each rounded); where loglik0 is not
 *     finite the chain has failed (it never moves again) and its logw is NaN from here on
 * Nothing requires the ladder to be monotone.  log p(t) is log_mean_w of logw when beta0 = 0 and beta[T - 1] = 1.
 * Outputs (host, each may be NULL): logw_out [n]; theta_out [n][D]: the last positions; accept_trace [T]: accepted proposals of the stage
 * / (n stage_len[k]); partial_out [5]: the partial of logw (rmhmc_ais_partial_dev); seconds_out: host wall time of the call.
 * Positions, logw and the chain records stay on the device between stages; the context is left with the last mass installed, and like
 * every sampling call the run invalidates the chain state.  The call equals the composition of the public pieces above, run by the
 * caller with the same seeds, bit for bit.
 * RMHMC_ERR_INVALID: T < 1, a NULL beta or stage_len, a stage shorter than 1, a stage_mass entry other than 0 / 1, a stage_mass entry of 1
 * with H_lik NULL, a beta or beta0 that is not finite or < 0, theta0 NULL with beta0 != 0, L < 1, no mass set. */
int rmhmc_ais_run(rmhmc_ctx *ctx, const double *theta0, double beta0, int32_t T, const double *beta, const int64_t *stage_len,
                  const int32_t *stage_mass, const double *H_lik, int32_t L, double eps, uint64_t seed, int64_t chain_offset,
                  double *logw_out, double *theta_out, double *accept_trace, double *partial_out, double *seconds_out);

#ifdef __cplusplus
}
#endif

#endif /* RMHMC_AIS_H */
