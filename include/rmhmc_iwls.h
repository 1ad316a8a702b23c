/*
 * rmhmc_iwls.h — C-ABI of the IWLS Metropolis-Hastings sampler of the reference, code/iwls.py:13-89, on the MI355X
 * (librmhmc_hip.so).  Same context, data and conventions as rmhmc.h (host buffers, float64, chain-major, int status,
 * rmhmc_last_error).  Kept out of rmhmc.h: the CPU oracle does not implement it.
 *
 * Semantics (per chain): w = theta0 (default 0), prior N(0, alpha I) of rmhmc_set_data, G(w) = X'WX + I/alpha = L L',
 * W = p(1-p), p = 1/(1+e^-f), f = X w.  Every iteration proposes w' = m(w) + L^-T z, z ~ N(0, I), m(w) = w + G^-1 grad(w) (the
 * reference's current_mean), and accepts iff ratio > 0 or ratio > log(u), u read only when ratio > 0 is false, with
 *   ratio = LJL(w') + log q(w | w') - LJL(w) - log q(w' | w),   log q(x | w) = l(w) - |L'(x - m(w))|^2 / 2.
 * compat != 0 (the reference): l(w) = -sum log diag chol(G^-1 + 1e-6 I), and a proposal is "saturated" - ratio = NaN, rejected, as
 * the reference's 0/0 in inv_W = eye/W - when some row has W_j == 0 or a non-finite 1/W_j (fp64, the expressions above).  The
 * reference therefore samples a truncated posterior (no row with f_j > 36.7).  compat == 0: l(w) = sum log diag L, no saturation
 * rule.  Both: the naive log(1 + exp f) (LJL = -inf where exp overflows: rejected); a record at w' that is not positive definite is
 * rejected.  D <= 64 (RMHMC_ERR_UNSUPPORTED beyond).  Kernels and random streams: riemannhamiltonianmontecarlo_amd/csrc/iwls.hip.h.
 */
#ifndef RMHMC_IWLS_H
#define RMHMC_IWLS_H

#include "rmhmc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sample n_iter iterations of every chain with the library's Philox streams, chain c keyed by (seed, chain_offset + c).
 * samples_out [n][n_iter - burn_in][D]: row k = w after iteration burn_in + k (every row is written, iwls.py:84-85).
 * accepted_out [n]: accepted proposals of the whole run; saturated_out [n]: saturated proposals (compat; 0 otherwise); seconds_out:
 * wall time from the top of iteration burn_in to the end of the last iteration (iwls.py:41-43,88).  A progress callback
 * (rmhmc_set_progress; its first / every are not used) is called with RMHMC_EV_PROGRESS and i before iteration i for every
 * i % 1000 == 0, then with RMHMC_EV_BURNIN_DONE and burn_in before iteration burn_in (accepted_total: summed over the chains);
 * the timer starts after those calls.  theta0 [n][D], accepted_out, saturated_out and seconds_out may be NULL.
 * 0 <= burn_in < n_iter < 2^32.
 * Equivalent to rmhmc_iwls_sample_to (rmhmc_out.h) with the descriptor {RMHMC_OUT_HOST, samples_out}. */
int rmhmc_iwls_sample(rmhmc_ctx *ctx, int64_t n_iter, int64_t burn_in, int32_t compat, uint64_t seed, int64_t chain_offset,
                      const double *theta0, double *samples_out, int64_t *accepted_out, int64_t *saturated_out,
                      double *seconds_out);

/* The same kernels fed with given proposals instead of drawn ones (the reference draws them by SVD): w_prop [n][n_iter][D],
 * u [n][n_iter] (NaN where the reference drew none).  After every iteration: w_out [n][n_iter][D], mean_out [n][n_iter][D]
 * (current_mean), ljl_out, ratio_out [n][n_iter]; decisions_out [n][n_iter]: bit 0 accepted, bit 1 u read, bit 2 saturated.
 * theta0, mean_out, ljl_out, ratio_out and decisions_out may be NULL.  0 < n_iter < 2^32. */
int rmhmc_iwls_replay(rmhmc_ctx *ctx, int64_t n_iter, int32_t compat, const double *w_prop, const double *u,
                      const double *theta0, double *w_out, double *mean_out, double *ljl_out, double *ratio_out,
                      int8_t *decisions_out);

#ifdef __cplusplus
}
#endif

#endif /* RMHMC_IWLS_H */
