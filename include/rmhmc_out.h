/*
 * rmhmc_out.h — C-ABI of the output descriptor: every sampler of librmhmc_hip.so with its samples left
 * in device memory, reduced on the device, or both.  Same context, data and conventions as rmhmc.h.
 * Kept out of rmhmc.h: the CPU oracle does not implement it.
 *
 * A *_sample_to call runs the sampler of the matching *_sample entry point: for equal run arguments the
 * samples and counters are bit-identical, the context is left as that call leaves it, and seconds_out
 * covers what it covers there (the reductions run after the timer stops).  The descriptor is passed per
 * call; the context keeps none of it.
 *
 * Refused before any sampling work: a NULL descriptor, one that requests no output, or a `where` that
 * is neither constant (RMHMC_ERR_INVALID); a statistic (mean, var, ess, run_mean, run_ess) with
 * n_iter - burn_in outside 2..20000 (RMHMC_ERR_UNSUPPORTED: the ESS kernel holds one series in LDS;
 * samples alone have no such limit).  The limits of each sampler are those of its *_sample entry point.
 * On return the library's stream is idle: any stream may read the device outputs.  The library works on a
 * stream of its own that is not ordered against any other: work of the caller that writes a device
 * buffer handed to these functions (an input of rmhmc_ess_dev, or a fill of an output) must have finished
 * before the call.  rmhmc_kernel_time(ctx, "write_out", &s, NULL) returns the host wall time of the last
 * call's write-out (copies and reductions, from the end of the sampling to the idle stream).  The older
 * *_sample, *_sample_dev and *_sample_stats[_dev] entry points write out the same way (each is the
 * *_sample_to call with a descriptor of its own, named at its declaration), so the figure reflects them too.
 */
#ifndef RMHMC_OUT_H
#define RMHMC_OUT_H

#include "rmhmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RMHMC_OUT_HOST   0
#define RMHMC_OUT_DEVICE 1          /* plain device pointers of the context's GPU, e.g. tensor.data_ptr() */
typedef struct {
  int32_t where;                    /* memory space of EVERY pointer below and of the per-call counter outputs */
  double *samples;                  /* [n][S][D], S = n_iter - burn_in                                 or NULL */
  double *mean, *var, *ess;         /* [n][D] each: what rmhmc_sample_stats returns                    or NULL */
  double *run_mean;                 /* [S][D]: mean over the n chains of sample row s                  or NULL */
  double *run_ess;                  /* [D]: ESS of the columns of run_mean                             or NULL */
} rmhmc_out;

/* mean, var, ess: the ESS kernel of rmhmc_ess / rmhmc_sample_stats on the samples of the call (mean and
 * population variance per chain and dimension; RMHMC_FLAG_ESS_WRAP of the context selects the FFT-length
 * convention).  run_mean[s][d] = (sum over c = 0..n-1, in that order, of samples[c][s][d]) / n; run_ess:
 * the same ESS kernel on run_mean as one series block of S x D.  NaN propagates: a Gibbs chain that
 * stopped has NaN rows, so its mean / var / ess and the rows of run_mean it touches are NaN.  The same
 * holds for a series with an inf: mean, var and ess are all NaN (not the +-inf of the sum).  A constant
 * series has its mean, var = 0 and ess = NaN.
 *
 * The counters ([n] int64 unless noted, each may be NULL) live in the memory space `where` names;
 * seconds_out is a host scalar. */

/* rmhmc_sample (rmhmc.h) */
int rmhmc_sample_to(rmhmc_ctx *ctx, int64_t n_iter, int64_t burn_in, int32_t L, double eps, int32_t K, uint64_t seed,
                    int64_t chain_offset, const double *theta0, const rmhmc_out *out, int64_t *accept_out,
                    int64_t *steps_out, double *seconds_out);
/* rmhmc_hmc_sample (rmhmc.h) */
int rmhmc_hmc_sample_to(rmhmc_ctx *ctx, int64_t n_iter, int64_t burn_in, int32_t L, double eps, uint64_t seed,
                        int64_t chain_offset, const double *theta0, const rmhmc_out *out, int64_t *accept_out,
                        int64_t *steps_out, double *seconds_out);
/* rmhmc_mmala_sample (rmhmc.h) */
int rmhmc_mmala_sample_to(rmhmc_ctx *ctx, int64_t n_iter, int64_t burn_in, double eps, uint64_t seed,
                          int64_t chain_offset, const double *theta0, const rmhmc_out *out, int64_t *accept_out,
                          double *seconds_out);
/* rmhmc_amh_sample (rmhmc_amh.h); sd_out [n][D] double */
int rmhmc_amh_sample_to(rmhmc_ctx *ctx, int64_t n_iter, int64_t burn_in, uint64_t seed, int64_t chain_offset,
                        const double *theta0, const rmhmc_out *out, int64_t *accepted_out, double *sd_out,
                        double *seconds_out);
/* rmhmc_iwls_sample (rmhmc_iwls.h) */
int rmhmc_iwls_sample_to(rmhmc_ctx *ctx, int64_t n_iter, int64_t burn_in, int32_t compat, uint64_t seed,
                         int64_t chain_offset, const double *theta0, const rmhmc_out *out, int64_t *accepted_out,
                         int64_t *saturated_out, double *seconds_out);
/* rmhmc_gibbs_sample (rmhmc_gibbs.h) without its Z_out / lam_out */
int rmhmc_gibbs_sample_to(rmhmc_ctx *ctx, int64_t n_iter, int64_t burn_in, uint64_t seed, int64_t chain_offset,
                          const rmhmc_out *out, int64_t *capped_out, int64_t *stopped_out, double *seconds_out);

/* The ESS kernel on samples already in device memory, samples_dev [n][S][P] -> ess_dev, mean_dev,
 * var_dev [n][P] in device memory; each output may be NULL, not all three.  2 <= S <= 20000. */
int rmhmc_ess_dev(rmhmc_ctx *ctx, const double *samples_dev, int64_t n, int64_t S, int32_t P, double *ess_dev,
                  double *mean_dev, double *var_dev);

#ifdef __cplusplus
}
#endif

#endif /* RMHMC_OUT_H */
