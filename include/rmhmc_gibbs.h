/*
 * rmhmc_gibbs.h — C-ABI of the auxiliary-variable Gibbs sampler of the reference (Holmes and Held), code/gibbs_sampler.py:14-139, on
 * the MI355X (librmhmc_hip.so).  Same context, data and conventions as rmhmc.h (host buffers, float64, chain-major, int status,
 * rmhmc_last_error).  Kept out of rmhmc.h: the CPU oracle does not implement it.
 *
 * Semantics (per chain; N = the context's M rows, prior N(0, v I) with v = the alpha of rmhmc_set_data): latent Z [N], mixing weights
 * lam [N] (start 1), beta [D].  Z_j starts as N(0, 1) truncated to (0, inf) where t_j = 1 and to (-inf, 0) where t_j = 0.  Every
 * iteration: V = (X' diag(1/lam) X + I/v)^-1, L = chol(V), B = V X'(Z/lam); the sweep over the rows j = 0..N-1 in order
 * (h_j = x_j'V x_j, w_j = h_j/(lam_j - h_j), m = x_j.B, m -= w_j (Z_j - m), Z_j ~ N(m, lam_j (w_j + 1)) truncated by t_j,
 * B += (Z_j - z_old)/lam_j V x_j); beta = B + L T, T ~ N(0, I); then for every row one draw of lam_j by the reference's rejection
 * sampler at r = |Z_j - x_j.beta|, with both of its alternating series as the Python file writes them.
 *
 * D <= 64 (RMHMC_ERR_UNSUPPORTED beyond).  fp64 throughout: the weighted Gram matrix is assembled on the fp64 matrix cores whatever
 * the int8 metric flags of the context say (they are ignored by this sampler).  chain_offset + n_chains <= 2^32.
 * Bounds (the reference has none): 64 attempts per row and draw of lam_j, 64 pairs of terms per series test; a row that reaches one
 * keeps its last proposal and adds one to its chain's capped counter.  Work is launched without host synchronisation between the
 * iterations the reference reports on (i % 100 == 0) and iteration burn_in.  Kernels and random streams:
 * riemannhamiltonianmontecarlo_amd/csrc/gibbs.hip.h.
 */
#ifndef RMHMC_GIBBS_H
#define RMHMC_GIBBS_H

#include "rmhmc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sample n_iter iterations of every chain with the library's Philox streams, chain c keyed by (seed, chain_offset + c).
 * samples_out [n][n_iter - burn_in][D]: row k = beta of iteration burn_in + k (every row is written, gibbs_sampler.py:130-131).
 * capped_out [n]: rows that reached a bound of the mixing-weight sampler (expected 0).  stopped_out [n]: -1, or the iteration whose draw
 * of some lam_j was not a positive finite number (the reference's formula for its proposal cancels for residuals below about 1e-7 and
 * can return lam_j = inf: about 3e-9 of all draws; the reference itself ends in a ValueError in its next sweep): that chain stops
 * there, its later rows of samples_out are NaN.  seconds_out: wall time from the top of
 * iteration burn_in to the end of the last iteration (:100-101,137).  A progress callback (rmhmc_set_progress; its first / every are
 * not used) is called with RMHMC_EV_PROGRESS and i before every iteration i % 100 == 0 (:97-98); the timer starts after the call
 * at burn_in.  Z_out and lam_out [n][N]: the state after the last iteration (of a stopped chain: the state it stopped in).  capped_out,
 * stopped_out, Z_out, lam_out and seconds_out may be NULL.  0 <= burn_in < n_iter < 2^32.
 * Equivalent to rmhmc_gibbs_sample_to (rmhmc_out.h) with the descriptor {RMHMC_OUT_HOST, samples_out}, plus Z_out and lam_out. */
int rmhmc_gibbs_sample(rmhmc_ctx *ctx, int64_t n_iter, int64_t burn_in, uint64_t seed, int64_t chain_offset, double *samples_out,
                       int64_t *capped_out, int64_t *stopped_out, double *Z_out, double *lam_out, double *seconds_out);

/* The same kernels fed from recorded draws: u_init [n][N] (the uniform behind the initial Z_j, by row), u_sweep [n][n_iter][N] (the
 * uniform behind every draw of the sweep), T [n][n_iter][D], ks_draws [n][ks_total][3] (normal, uniform, uniform of every attempt of
 * the mixing-weight sampler) and ks_offset [n][n_iter][N+1]: row j of iteration i owns the attempts ks_offset[i][j] ..
 * ks_offset[i][j+1] - 1 of its chain (non-decreasing, within 0..ks_total).  After every iteration: beta_out and B_out [n][n_iter][D]
 * (B before the T term), attempts_out [n][n_iter][N] (attempts each row consumed); after the last: Z_out and lam_out [n][N].
 * status_out [n]: 0; 1 where the device wanted more attempts for a row than the tape holds; 2 where a draw of lam_j was not a positive
 * finite number: that chain stops there, nothing is read past the row's draws.  The records of the iterations after the stop stay 0;
 * attempts_out, Z_out and lam_out of the stopping iteration itself are unspecified for the rows behind the one that stopped the chain
 * (the rows of an iteration are drawn concurrently).  capped_out as above.  Z_out, lam_out, capped_out and status_out may be NULL.
 * 0 < n_iter < 2^32. */
int rmhmc_gibbs_replay(rmhmc_ctx *ctx, int64_t n_iter, const double *u_init, const double *u_sweep, const double *T,
                       const double *ks_draws, const int64_t *ks_offset, int64_t ks_total, double *beta_out, double *B_out,
                       int32_t *attempts_out, double *Z_out, double *lam_out, int64_t *capped_out, int32_t *status_out);

#ifdef __cplusplus
}
#endif

#endif /* RMHMC_GIBBS_H */
