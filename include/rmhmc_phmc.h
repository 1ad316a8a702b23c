/*
 * rmhmc_phmc.h — C-ABI of HMC with a fixed dense mass matrix shared by all chains ("preconditioned HMC") on the
 * MI355X (librmhmc_hip.so), and of the damped Newton search for the posterior mode whose metric is the usual
 * choice of that matrix.  Same context, data and conventions as rmhmc.h (host buffers, float64, chain-major,
 * int status, rmhmc_last_error); the output descriptor is that of rmhmc_out.h.  Kept out of rmhmc.h: the CPU
 * oracle does not implement it.  Kernels: riemannhamiltonianmontecarlo_amd/csrc/phmc.hip.h.
 *
 * One transition of chain c, with Mass = Lm Lm' (Lm the lower Cholesky factor), LJL and grad as everywhere else
 * (the naive log(1 + exp f) included):
 *   start   z ~ N(0, I_D), p = Lm z, H_cur = -LJL(w) + z'z / 2, ns = ceil(u_len L); no direction flip
 *   ns steps   p += eps/2 grad(w); a NaN in p ends the trajectory here (RMHMC_ST_NONFINITE, the proposal is
 *           rejected); w += eps Mass^-1 p; grad, LJL at the new w; p += eps/2 grad(w)
 *   end     H_prop = -LJL(w*) + p' Mass^-1 p / 2, ratio = H_cur - H_prop, accept iff ratio > 0 or
 *           ratio > log(u_acc); a NaN ratio rejects
 * A chain whose H_cur or H_prop is not finite FAILS in the sense of rmhmc.h (its log joint has overflowed):
 * RMHMC_ST_NONFINITE, rejected, state untouched, neighbours unaffected.
 * Random streams: those of rmhmc_hmc_sample (normals of blocks d/2, u_len and u_acc the two values of block
 * 0x40000000 at counter (chain id, iteration), key (seed, chain_offset + c)).  With the identity as mass matrix
 * positions, momenta, Hamiltonians, step counts and decisions are those of rmhmc_hmc_* on its multi-launch
 * path, bit for bit.
 */
#ifndef RMHMC_PHMC_H
#define RMHMC_PHMC_H

#include "rmhmc_out.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Mass matrix of the context: mass[D*D], host, row-major, symmetric positive definite (the lower triangle is read).
 * NULL: identity.  Factorised on the host; RMHMC_ERR_INVALID for a non-finite entry or a pivot <= 0.  It stays until
 * the next call; rmhmc_set_data does not touch it. */
int rmhmc_phmc_set_mass(rmhmc_ctx *ctx, const double *mass);

/* Posterior mode by damped Newton from w0[D] (NULL: zeros).  w_out[D]; G_out[D*D] | NULL: the metric at w_out;
 * iters_out | NULL; step_out | NULL: max|s| of the last step.  RMHMC_OK whether or not it converged: the caller
 * compares *step_out with its tol.  Invalidates the chain state like rmhmc_metric.
 * Each iteration: s = G(w)^-1 grad(w), G = X' Lambda X + I / alpha; stop when max|s| <= tol max(1, max|w|) (the step is
 * not taken) or after max_iter steps; otherwise w += s / 2^k for the first k = 0..20 whose LJL is finite and >= LJL(w);
 * if there is none, stop. */
int rmhmc_phmc_mode(rmhmc_ctx *ctx, const double *w0, int32_t max_iter, double tol, double *w_out, double *G_out,
                    int32_t *iters_out, double *step_out);

/* One transition with caller-supplied randomness; arguments as rmhmc_hmc_transition plus status_out[n] | NULL. */
int rmhmc_phmc_transition(rmhmc_ctx *ctx, double *w, const double *z, const double *u_len, const double *u_acc,
                          int32_t L, double eps, int32_t *accepted_out, int32_t *nsteps_out, double *H_cur_out,
                          double *H_prop_out, double *w_prop_out, double *p_prop_out, int32_t *status_out);

/* The sampler, every output mode: arguments and contract as rmhmc_hmc_sample_to (theta0 NULL: zeros). */
int rmhmc_phmc_sample_to(rmhmc_ctx *ctx, int64_t n_iter, int64_t burn_in, int32_t L, double eps, uint64_t seed,
                         int64_t chain_offset, const double *theta0, const rmhmc_out *out, int64_t *accept_out,
                         int64_t *steps_out, double *seconds_out);

#ifdef __cplusplus
}
#endif

#endif /* RMHMC_PHMC_H */
