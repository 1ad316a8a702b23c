/*
 * rmhmc_loo.h — C-ABI of leave-one-out cross-validation in librmhmc_hip.so: Pareto-smoothed importance sampling (PSIS-LOO; Vehtari,
 * Simpson, Gelman, Yao, Gabry) and WAIC of a Bayesian logistic regression over the rows it was trained on, from posterior draws in
 * device memory, computed where the draws are.  Same context and conventions as rmhmc.h, rmhmc_pred.h and rmhmc_quant.h.  Kept out of
 * rmhmc.h: the CPU oracle does not implement it.  Kernels: riemannhamiltonianmontecarlo_amd/csrc/loo.hip.h; host half: csrc/loo.h.  The
 * specification below is restated line by line in np.longdouble in tests/helpers/loo_ref.py.
 *
 * Inputs.  samples_dev [n][S][D] in device memory (what every *_sample_to call of rmhmc_out.h writes): the N = n S rows are the draws
 * w_k.  x [C][D], host, every entry finite: the data rows, called columns here (a column of the log-likelihood matrix).  t [C], host,
 * required: every entry exactly 0.0 or 1.0.  The context is used for its device and stream only: the chain state and the training data
 * are not touched.
 *
 * Log-likelihood.  For column c and draw k: f = x_c . w_k, s = f if t_c = 1 else -f, e = exp(-|f|), l = min(s, 0) - log1p(e): no
 * log(1 - p) by subtraction, so l keeps its relative accuracy from -1e-300 to -800.  -0.0 is written as +0.0.  A draw with any
 * non-finite entry gets NaN in every column, decided in a validity pass of its own (as in rmhmc_pred.h: an infinite w_k times x can give
 * a finite-looking f).  An f that is NaN gives NaN.  ll [n][S][C], N rows of C values.
 *
 * Every later stage leaves a non-finite l out of its own column.  m_c is the number of finite l of column c.
 *
 * Moments partial.  double[5 * C], rows of length C:
 *   row 0: m (an exact integer)   row 1: the mean of l   row 2: M2 = sum (l - mean)^2   row 3: SQ = sum exp(l)   row 4: lmin, the
 *   smallest l (+inf for m = 0; mean, M2 and SQ are 0 then)
 * The sums are compensated and in a fixed order that depends on N alone; no atomics.  Two partials merge by Chan's update of mean and
 * M2 (delta = mean_b - mean_a, m = m_a + m_b, mean = mean_a + delta m_b / m, M2 = M2_a + M2_b + delta^2 m_a m_b / m), addition of m and
 * SQ and the minimum of lmin; a partial with m = 0 is the identity, to the bit.
 * Finished: lppd_c = log(SQ / m), p_waic_c = M2 / (m - 1) (NaN for m < 2), elpd_waic_c = lppd_c - p_waic_c.
 *
 * Tail length (rmhmc_loo_plan, integers only).  M_c = min(floor(m_c / 5), r), r the smallest integer with r^2 >= 9 m_c: min(0.2 m,
 * 3 sqrt(m)), the PSIS rule at a relative efficiency of 1 (the autocorrelation of the draws is deliberately not used).  M_c < 5: no
 * smoothing, khat = +inf, target rank -1.  M_c > RMHMC_LOO_MAX_TAIL: RMHMC_ERR_UNSUPPORTED (the tail of a column is sorted and fitted
 * in LDS; that allows m up to 29 826 161 draws).
 *
 * Cutoff.  The log weights are lw = lmin - l <= 0 (the log ratio -l minus its maximum).  The tail of a column is its M_c smallest l.
 * The cutoff lcut is the order statistic of rank M_c (0-based, ascending) of the column's finite l, found with the exact select of
 * rmhmc_quant.h (rmhmc_quant_hist_dev on ll with P = C, rmhmc_quant_step, one target per column): bit for bit sort(ll[:, c])[M_c].
 *
 * Split.  n_lt = #{l < lcut}, n_gt = #{l > lcut}, n_eq = m - n_lt - n_gt, r = M_c - n_lt.  The tail holds the n_lt values below the
 * cutoff and r copies of lcut.  Body: A_body = sum over l > lcut of exp(lmin - l) + (n_eq - r) exp(lmin - lcut) (compensated, fixed
 * order, no atomics), B_body = (n_gt + n_eq - r) exp(lmin), because lw + l = lmin for every unsmoothed draw.  The values below the
 * cutoff are gathered into tail [C][stride] slots through one integer slot counter per column (atomic, like the counts of
 * rmhmc_quant.h); the sort of the fit makes the result independent of the order of arrival.  A column with M_c < 5 has no tail: all
 * its finite l are body (n_lt = 0, n_gt = m; its cut is not read).
 *
 * Fit.  Per column with M = M_c >= 5:
 *   1. the tail is sorted so that lw ascends: lw_1 <= .. <= lw_M, l_j the l of rank j.
 *   2. y_j = expm1(lw_j - lw_cut) >= 0, lw_cut = lmin - lcut: the generalised Pareto fit is scale-free, so the exceedances are taken
 *      relative to the cutoff weight, which stays accurate when lw_cut is -700.
 *   3. y_M = 0 or y_q = 0, q = floor(M / 4 + 0.5): the tail is constant or mostly tied; no smoothing, khat = +inf.
 *   4. otherwise Zhang and Stephens (2009) as PSIS uses it, G = 30 + floor(sqrt(M)), i = 1 .. G:
 *      theta_i = 1 / y_M + (1 - sqrt(G / (i - 0.5))) / (3 y_q), kappa_i = mean_j log1p(-theta_i y_j),
 *      L_i = M (log(-theta_i / kappa_i) - kappa_i - 1), omega_i = exp(L_i - max L) / sum exp(L - max L), theta = sum omega_i theta_i,
 *      k = mean_j log1p(-theta y_j), sigma = -k / theta, khat = (k M + 5) / (M + 10) (ten pseudo-observations at 0.5).
 *   5. khat or sigma not finite: no smoothing, khat = +inf.
 *   6. smoothed tail, p_j = (j - 0.5) / M: q_j = sigma expm1(-khat log1p(-p_j)) / khat (-sigma log1p(-p_j) for khat = 0),
 *      lw'_j = min(lw_cut + log1p(q_j), 0).  Weights are paired with draws by rank: draw j keeps its own l_j.
 *   7. A_tail = sum exp(lw'_j), B_tail = sum exp(lw'_j + l_j), compensated sums in a fixed order.
 *   8. without smoothing lw' = lw.
 * fit [4 * C], rows of length C: khat, sigma, A_tail, B_tail.  M_c < 5: +inf, NaN, 0, 0.
 *
 * Finish (host).  elpd_loo_c = log(B_tail + B_body) - log(A_tail + A_body), p_loo_c = lppd_c - elpd_loo_c.  Totals in column order.
 * se = sqrt(C var), var the sample variance (C - 1) of the pointwise values, for elpd_loo and elpd_waic; NaN for C < 2.  The number of
 * khat in (0.5, 0.7] and above 0.7 (an infinite khat counts as above).  m = 0: NaN.
 */
#ifndef RMHMC_LOO_H
#define RMHMC_LOO_H

#include "rmhmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RMHMC_LOO_MAX_COLS 64    /* most columns of one device call: the widest column tile of the select */
#define RMHMC_LOO_MAX_TAIL 16384 /* longest tail of a column: 128 KB of LDS */

/* Stream and synchronisation of every *_dev call as rmhmc_ess_dev of rmhmc_out.h: the inputs must be complete before the call, the
 * library's stream is idle on return.  Every refusal is decided on the host before any device work, with the outputs untouched:
 * RMHMC_ERR_INVALID for a NULL pointer, n, S, D or C < 1, C > RMHMC_LOO_MAX_COLS, a non-finite entry of x, an entry of t other than 0 or
 * 1, a tail length outside 0 .. min(stride, RMHMC_LOO_MAX_TAIL); RMHMC_ERR_UNSUPPORTED for D > 256. */

/* samples_dev [n][S][D], x [C][D], t [C] -> ll_dev [n][S][C] (device memory).  The l of a (draw, column) pair does not depend on where
 * the draw or the column sits in the call. */
int rmhmc_loo_loglik_dev(rmhmc_ctx *ctx, const double *samples_dev, int64_t n, int64_t S, int32_t D, const double *x, const double *t,
                         int32_t C, double *ll_dev);

/* ll_dev [n][S][C] -> partial_dev [5 * C] (device memory) */
int rmhmc_loo_moments_dev(rmhmc_ctx *ctx, const double *ll_dev, int64_t n, int64_t S, int32_t C, double *partial_dev);

/* Host only, no context: m [C] -> tail_len [C] = M_c and rank [C] = M_c, or -1 where M_c < 5.  RMHMC_ERR_INVALID for a NULL pointer,
 * C < 1 or a negative m; RMHMC_ERR_UNSUPPORTED for an M_c above RMHMC_LOO_MAX_TAIL; nothing is written then. */
int rmhmc_loo_plan(const int64_t *m, int32_t C, int64_t *tail_len, int64_t *rank);

/* ll_dev [n][S][C]; cut [C], lmin [C], tail_len [C]: host -> tail_dev [C][stride] (the first n_lt slots of a row are written),
 * counts_dev [2 * C] (int64: n_lt, n_gt), body_dev [2 * C] (A_body, B_body), all device memory.  stride >= 1. */
int rmhmc_loo_split_dev(rmhmc_ctx *ctx, const double *ll_dev, int64_t n, int64_t S, int32_t C, const double *cut, const double *lmin,
                        const int64_t *tail_len, int64_t stride, double *tail_dev, int64_t *counts_dev, double *body_dev);

/* tail_dev [C][stride] and counts_dev [2 * C] of the split (device memory), cut, lmin, tail_len: host -> fit_dev [4 * C] (device) */
int rmhmc_loo_fit_dev(rmhmc_ctx *ctx, const double *tail_dev, const int64_t *counts_dev, const double *cut, const double *lmin,
                      const int64_t *tail_len, int64_t stride, int32_t C, double *fit_dev);

/* Host only, no context: merges the k moments partials (host pointers, all of C columns) in the order given and finishes with
 * fit [4 * C] and body [2 * C] (host; both NULL: WAIC alone, the LOO outputs are NaN).  Outputs, host, each may be NULL: merged [5 * C]
 * (not one of the partials), elpd_loo, p_loo, pareto_k, lppd, p_waic, elpd_waic [C], totals [6] = elpd_loo, se_elpd_loo, p_loo,
 * elpd_waic, se_elpd_waic, p_waic, k_counts [2] = khat in (0.5, 0.7], khat above 0.7, draws_used [C] = m.  RMHMC_ERR_INVALID, nothing
 * written, for k < 1, C < 1, a NULL partial or only one of fit and body. */
int rmhmc_loo_finish(const double *const *partials, int32_t k, int64_t C, const double *fit, const double *body, double *merged,
                     double *elpd_loo, double *p_loo, double *pareto_k, double *lppd, double *p_waic, double *elpd_waic, double *totals,
                     int64_t *k_counts, int64_t *draws_used);

/* The whole run over the R rows x [R][D], t [R] in blocks of cols_per_block columns (1 .. 64; 0: the largest power of two <= 64 whose
 * ll block of N cols_per_block doubles stays within 2 GiB, at least 1), with one scratch allocation.  partial [5 * R], fit [4 * R],
 * body [2 * R]: host, each may be NULL; the other outputs as rmhmc_loo_finish with C = R.  Equal bit for bit to rmhmc_loo_loglik_dev,
 * rmhmc_loo_moments_dev, rmhmc_loo_plan, the eight rounds of rmhmc_quant_hist_dev / rmhmc_quant_step on ll, rmhmc_loo_split_dev,
 * rmhmc_loo_fit_dev on every block and one rmhmc_loo_finish, and the same bits for every cols_per_block.  Refusals as those calls,
 * R >= 1 of any size. */
int rmhmc_loo_dev(rmhmc_ctx *ctx, const double *samples_dev, int64_t n, int64_t S, int32_t D, const double *x, const double *t, int64_t R,
                  int32_t cols_per_block, double *partial, double *fit, double *body, double *elpd_loo, double *p_loo, double *pareto_k,
                  double *lppd, double *p_waic, double *elpd_waic, double *totals, int64_t *k_counts, int64_t *draws_used);

#ifdef __cplusplus
}
#endif

#endif /* RMHMC_LOO_H */
