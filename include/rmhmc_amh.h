/*
 * rmhmc_amh.h — C-ABI of the component-wise adaptive Metropolis sampler (AMH) of the reference,
 * code/metropolis.py:14-94, on the MI355X (librmhmc_hip.so).  Same context, data and conventions as
 * rmhmc.h (host buffers, float64, chain-major, int status, rmhmc_last_error).  Kept out of rmhmc.h:
 * the CPU oracle does not implement it.
 *
 * Semantics (per chain): w = theta0 (default 0), ProposalSD = 1, prior N(0, alpha I) of rmhmc_set_data.
 * Every iteration sweeps d = 0..D-1: wNew[d] = w[d] + z SD[d]; accept iff Ratio > 0 or Ratio > log(u),
 * u read only when Ratio > 0 is false.  At iterations i % 100 == 0, i < burn_in (i = 0 included, its
 * window is one proposal) SD[d] *= 1.2 where the window's acceptance ratio is > 0.5, *= 0.8 where it is
 * < 0.2; the counters are then reset.  The log-likelihood uses the naive log(1 + exp f), as the
 * reference does (inf where exp overflows; such proposals are rejected).
 *
 * Work is launched in segments of at most 1000 iterations, cut after the iterations the reference
 * reports on (i % 1000 == 0, i < burn_in) and after iteration burn_in.  Kernel and random streams:
 * riemannhamiltonianmontecarlo_amd/csrc/amh.hip.h.
 */
#ifndef RMHMC_AMH_H
#define RMHMC_AMH_H

#include "rmhmc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Sample n_iter iterations of every chain with the library's Philox streams, chain c keyed by
 * (seed, chain_offset + c).  samples_out [n][n_iter - burn_in][D]: row k = state after iteration
 * burn_in + k (the reference never writes its row 0, metropolis.py:67-68).  accepted_out [n]: accepted
 * proposals of the whole run; sd_out [n][D]: final ProposalSD; seconds_out: wall time of the iterations
 * after burn_in (metropolis.py:93-96).  A progress callback (rmhmc_set_progress) is called with
 * RMHMC_EV_PROGRESS and i after iteration i for i % 1000 == 0, i < burn_in, and with
 * RMHMC_EV_BURNIN_DONE and burn_in after iteration burn_in.  theta0 [n][D], accepted_out, sd_out and
 * seconds_out may be NULL.  0 <= burn_in < n_iter < 2^32.
 * Equivalent to rmhmc_amh_sample_to (rmhmc_out.h) with the descriptor {RMHMC_OUT_HOST, samples_out}. */
int rmhmc_amh_sample(rmhmc_ctx *ctx, int64_t n_iter, int64_t burn_in, uint64_t seed, int64_t chain_offset,
                     const double *theta0, double *samples_out, int64_t *accepted_out, double *sd_out,
                     double *seconds_out);

/* The same kernel fed from recorded draws: z and u [n][n_iter][D] (u NaN where the reference drew
 * none).  w_out [n][n_iter][D] and ljl_out [n][n_iter]: w and CurrentLJL after every iteration;
 * decisions_out [n][n_iter][D]: bit 0 accepted, bit 1 u was read; sd_out [n][D] final ProposalSD.
 * theta0 and sd_out may be NULL. */
int rmhmc_amh_replay(rmhmc_ctx *ctx, int64_t n_iter, int64_t burn_in, const double *z, const double *u,
                     const double *theta0, double *w_out, double *ljl_out, double *sd_out,
                     int8_t *decisions_out);

#ifdef __cplusplus
}
#endif

#endif /* RMHMC_AMH_H */
