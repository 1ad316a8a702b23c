/*
 * rmhmc_smc.h — C-ABI of the log marginal likelihood by adaptive sequential Monte Carlo in librmhmc_hip.so: the annealing of
 * rmhmc_ais.h on a ladder that the run chooses from the conditional ESS of its own weights (Zhou, Johansen and Aston 2016), with
 * systematic resampling on integers.  Same context and conventions as rmhmc_ais.h (host buffers unless a name ends in _dev, float64,
 * chain-major, int status, rmhmc_last_error).  Kept out of rmhmc.h: the CPU oracle does not implement it.  Kernels:
 * riemannhamiltonianmontecarlo_amd/csrc/smc.hip.h; host half: csrc/smc.h.  Every _dev call runs on the context's stream and
 * synchronises, as rmhmc_ais_partial_dev; none touches the chain state.
 *
 * Particles.  lw [n]: log weights; l [n]: loglik (rmhmc_ais.h) of the particles' current points.  A particle whose l is not finite has
 * failed: it is a particle of weight zero from the next reweighting on (lw = -inf), it counts, and a resampling replaces it.  lw = NaN
 * marks an entry that is left out of everything, as in rmhmc_ais.h; the run itself never makes one.
 *
 * 1. Conditional ESS.  For a step delta of the inverse temperature the incremental weight of particle i is exp(delta l_i), and
 *      cess(delta) / n = (sum_i W_i exp(delta l_i))^2 / (sum_i W_i  *  sum_i W_i exp(2 delta l_i)),   W_i = exp(lw_i),
 *    in (0, 1], 1 for equal l.  For candidates delta_j, j < J, 1 <= J <= 32, each finite and > 0, the partial is double[2 + 4 J] =
 *      (a0, S0, then per j: a1_j, S1_j, a2_j, S2_j)
 *    where (a, S) of a set of exponents x is a = max x and S = sum exp(x - a), and a = -inf, S = 0 if the set is empty or every x is -inf:
 *      (a0, S0)     of x = lw_i over the entries with lw_i not NaN
 *      (a1_j, S1_j) of x = lw_i + t_ij,   t_ij = delta_j l_i, over the entries with lw_i not NaN and l_i finite
 *      (a2_j, S2_j) of x = lw_i + 2 t_ij  over the same entries
 *    (a product and a sum, each rounded; 2 t is exact; no contraction).  Two partials merge per pair as the weight partials of
 *    rmhmc_ais.h: a = max(a', a''), S = S' exp(a' - a) + S'' exp(a'' - a); a pair with a = -inf is the identity.  Finished, with
 *    L = a + log S:   frac_j = exp(2 L1_j - L0 - L2_j) (evaluated left to right), NaN where S0 = 0 or S1_j = 0.
 *    The same call gives the same bits (no atomics; the order of every sum depends on n alone).  Rounding: a term's exponent carries the
 *    rounding of t, of the sum and of the subtraction of a, at most (|lw| + 2 |t| + 746) 2^-53, which is the relative error of the term.
 *
 * 2. The search for the next step.  SMC_ROUNDS = 3 rounds of SMC_J = 16 candidates, remaining = 1 - beta in (0, 1], rho in (0, 1):
 *      round 0      delta_j = remaining 8^-(15 - j) (exact scalings; the last is remaining itself); lo = 0
 *      rounds 1, 2  delta_j = lo + (hi - lo) ((j + 1) / 16) (a product and a sum, each rounded), the last is hi exactly
 *    In every round j* is the first j with frac_j < rho or frac_j NaN.  No such j in round 0: delta = remaining, flag LAST, frac = frac_15,
 *    and the search stops.  Otherwise hi = delta_j*, and lo = delta_(j* - 1) with its frac, or lo as it was for j* = 0; with no such j
 *    in a later round lo = hi = delta_15.  After round 2 delta = lo with the frac recorded for it; if lo is still 0, delta is the
 *    smallest candidate of round 0 with its frac there (which is below rho, or NaN) and flag FLOOR: the run always moves.
 *
 * 3. Reweighting.  lw_i <- lw_i + delta l_i where l_i is finite (a product and a sum, each rounded), -inf where it is not; NaN stays.
 *
 * 4. Systematic resampling on integers.  q_i = floor(2^40 exp(min(lw_i - a, 0))) as uint64, 0 for lw_i NaN or -inf, with a the maximum
 *    of the weight partial of rmhmc_ais.h (merged, for a sharded caller): 2^40 at the maximum.  With C_i the inclusive prefix sums of
 *    q, Q = C_n <= 2^60 and U a 32-bit unsigned,
 *      anc_j = min { i : C_i (n 2^32) > (j 2^32 + U) Q },   j = 0 .. n - 1, n <= 2^20,
 *    both sides below 2^112 and compared exactly.  This is systematic resampling with the offset U / 2^32 on the weights q / Q: anc is
 *    non-decreasing, the number of j with anc_j = i is floor(n q_i / Q) or that plus one, and equal q give anc_j = j.
 *
 * 5. The run: rmhmc_smc_run below.
 */
#ifndef RMHMC_SMC_H
#define RMHMC_SMC_H

#include "rmhmc_ais.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RMHMC_SMC_MAX_J 32          /* most candidates of one rmhmc_smc_cess_dev call */
#define RMHMC_SMC_J 16              /* candidates per round of the search */
#define RMHMC_SMC_ROUNDS 3          /* rounds of the search */
#define RMHMC_SMC_MAX_N 1048576     /* most particles of rmhmc_smc_ancestors_dev: 2^20 */
#define RMHMC_SMC_QBITS 40          /* q = 2^40 at the largest weight */
/* flags of a stage (flags_out) */
#define RMHMC_SMC_LAST 1            /* the step reaches beta = 1 */
#define RMHMC_SMC_FLOOR 2           /* no candidate met rho: the smallest was taken */
#define RMHMC_SMC_RESAMPLED 4       /* the stage resampled */

/* The partial of section 1: logw_dev [n], ll_dev [n] (device memory), delta [J] (host) -> partial_dev [2 + 4 J] (device memory).
 * RMHMC_ERR_INVALID for a NULL pointer, n < 1, J outside 1 .. 32 or a delta that is not finite and > 0. */
int rmhmc_smc_cess_dev(rmhmc_ctx *ctx, const double *logw_dev, const double *ll_dev, int64_t n, int32_t J, const double *delta,
                       double *partial_dev);

/* Host only, no context: merges the k partials (host pointers, [2 + 4 J] each) in the order given and finishes.  merged [2 + 4 J] | NULL,
 * frac [J] | NULL.  RMHMC_ERR_INVALID for k < 1, J outside 1 .. 32 or a NULL partial. */
int rmhmc_smc_cess_finish(const double *const *partials, int32_t k, int32_t J, double *merged, double *frac);

/* The search of section 2 on logw_dev [n], ll_dev [n] (device memory): three calls of rmhmc_smc_cess_dev's body and three downloads.
 * delta_out | NULL, frac_out | NULL, flags_out | NULL (host).  RMHMC_ERR_INVALID for a NULL input, n < 1, remaining outside (0, 1]
 * or rho outside (0, 1). */
int rmhmc_smc_choose_delta_dev(rmhmc_ctx *ctx, const double *logw_dev, const double *ll_dev, int64_t n, double remaining, double rho,
                               double *delta_out, double *frac_out, int32_t *flags_out);

/* Section 3, in place on logw_dev [n].  RMHMC_ERR_INVALID for a NULL pointer, n < 1 or a delta that is not finite. */
int rmhmc_smc_reweight_dev(rmhmc_ctx *ctx, double *logw_dev, const double *ll_dev, int64_t n, double delta);

/* q of section 4: logw_dev [n] -> q_dev [n] (uint64, device memory).  RMHMC_ERR_INVALID for a NULL pointer, n < 1 or a = NaN. */
int rmhmc_smc_quantise_dev(rmhmc_ctx *ctx, const double *logw_dev, int64_t n, double a, uint64_t *q_dev);

/* anc of section 4: q_dev [n] (every entry <= 2^40) -> anc_dev [n] (int32, device memory).  RMHMC_ERR_INVALID for a NULL pointer,
 * n < 1, an entry above 2^40 or Q = 0; RMHMC_ERR_UNSUPPORTED for n > 2^20.  A refusal writes nothing to anc_dev. */
int rmhmc_smc_ancestors_dev(rmhmc_ctx *ctx, const uint64_t *q_dev, int64_t n, uint32_t U, int32_t *anc_dev);

/* The run.  The context has its data and a mass, as for rmhmc_ais_run.  The positions start at theta0 [n][D], or for NULL at
 * rmhmc_ais_prior(seed, chain_offset), which requires beta0 = 0; logw = 0, logZ_acc = 0, beta = beta0, and one initial evaluation at
 * beta0 leaves l at the start positions.  Stage k = 0, 1, .. while beta < 1 and k < T_max:
 *   1. (delta_k, cess_k, flags) by section 2 from (logw, l) with remaining = 1 - beta and rho; beta_k = beta + delta_k, exactly 1 under LAST
 *   2. logw by section 3; its weight partial (rmhmc_ais_partial_dev) finished: log_mean_w, weight_ess = ess_k
 *   3. if ess_k < tau n: logZ_acc += log_mean_w; U = the high 32 bits of splitmix64(seed + 0x9E3779B97F4A7C15 (k + 1)) (mod 2^64,
 *      computed on the host); q by section 4 with the partial's maximum, anc from (q, U); particle j takes the position of anc_j;
 *      logw = 0; flag RESAMPLED.  Otherwise the positions stay.  (tau = 0 never resamples: annealed importance sampling on an
 *      adaptive ladder.  A weight_ess that is NaN - every weight zero - does not resample either.)
 *   4. if mass_every > 0 and (k is a multiple of mass_every or the stage is LAST): Mass = beta_k H_lik + I / alpha, as in rmhmc_ais_run;
 *      a refusal keeps the previous mass
 *   5. stage_len iterations of rmhmc_tphmc_sample_to's body at beta_k with burn_in = 0, seed + 1 + k (mod 2^64) and chain_offset from
 *      those positions (every particle starts afresh: status and counters at zero); l becomes loglik at the last states; beta = beta_k
 * where splitmix64(x): z = x + 0x9E3779B97F4A7C15; z = (z ^ z >> 30) 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) 0x94D049BB133111EB; z ^ z >> 31.
 * Result: log_z = logZ_acc + log_mean_w of the last logw; NaN if T_max stages have not reached beta = 1 (the call still returns
 * RMHMC_OK with the traces filled).  se: rmhmc_ais_finish's of the last logw if no stage resampled, NaN otherwise (resampled weights
 * are not independent).
 * Outputs (host, each may be NULL): T_out: stages taken; per stage [T_max], filled up to T_out: beta_out, cess_out, ess_out, flags_out,
 * accept_trace (as rmhmc_ais_run); logw_out [n]; theta_out [n][D]; log_z_out; se_out; partial_out [5]: the weight partial of the last
 * logw; seconds_out.  The context is left as rmhmc_ais_run leaves it.  The call equals the composition of the public pieces, run by
 * the caller with the same seeds, bit for bit.
 * RMHMC_ERR_INVALID: rho outside (0, 1), tau outside [0, 1], T_max < 1, stage_len < 1, mass_every < 0, mass_every > 0 with H_lik NULL,
 * beta0 not finite or outside [0, 1), theta0 NULL with beta0 != 0, L < 1, no mass set.  RMHMC_ERR_UNSUPPORTED: tau > 0 with more than
 * 2^20 chains.  All are decided before any device work. */
int rmhmc_smc_run(rmhmc_ctx *ctx, const double *theta0, double beta0, double rho, double tau, int32_t T_max, int64_t stage_len,
                  int64_t mass_every, const double *H_lik, int32_t L, double eps, uint64_t seed, int64_t chain_offset, int32_t *T_out,
                  double *beta_out, double *cess_out, double *ess_out, int32_t *flags_out, double *accept_trace, double *logw_out,
                  double *theta_out, double *log_z_out, double *se_out, double *partial_out, double *seconds_out);

#ifdef __cplusplus
}
#endif

#endif /* RMHMC_SMC_H */
