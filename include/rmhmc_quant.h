/*
 * rmhmc_quant.h — C-ABI of the posterior quantiles of librmhmc_hip.so: exact order statistics, and the quantiles interpolated between
 * them, of every dimension of the samples of many chains, computed where the samples are.  Same context and conventions as rmhmc.h.
 * Kept out of rmhmc.h: the CPU oracle does not implement it.
 *
 * samples [n][S][P] (what every *_sample_to call of rmhmc_out.h writes, P = D), read as N = n S rows of P values.
 *
 * Key.  key(x) is an order-preserving bijection from the finite doubles to uint64: -0.0 is first made +0.0; then, of the bit pattern
 * of x, all bits are inverted where the sign bit is set, and the sign bit is set where it is not.  x < y exactly when
 * key(x) < key(y); the inverse undoes the second step, so a returned zero is +0.0.
 *
 * Non-finite values.  A NaN or an infinity is left out of its own dimension only, as in rmhmc_diag.h.  m_d is the number of finite
 * values of dimension d over all N rows: the total of the round-0 histogram of d.
 *
 * Rounds.  An order statistic is found by a radix select on the key in eight rounds r = 0 .. 7; round r looks at the key bits
 * 63-8r .. 56-8r (the digit of the round).  A target is a (rank, dimension) pair: K ranks per dimension, each with a 64-bit prefix
 * [K][P] and a remaining rank [K][P].  In round r a value of dimension d belongs to target k when the top 8r bits of its key equal
 * those of prefix[k][d]; round 0 has no prefix, and its one histogram per dimension serves every target.  After round r the top
 * 8(r+1) bits of a prefix are the digits chosen so far; after round 7 the prefix is the key of the order statistic.  Between rounds
 * the 56-8r bits below the digits are not part of the prefix: they carry min(c, 2^(56-8r) - 1), c the count of the bin chosen in
 * round r, which is how the next step recognises a histogram that does not belong to it.  The device call ignores them.
 *
 * Histogram partial.  double[Kh][P][256], Kh = 1 in round 0 and K afterwards: entry [k][d][b] is the number of finite values of
 * dimension d that belong to target k and whose digit is b, an exact integer stored as a double (like row 0 of the diag partial).
 * Two partials merge by addition; all zeros is the identity.  The counts are integers (below 2^53), so the same bits result from
 * any split of the chains over shards and from any order of accumulation: this is the one partial of the library that is summed with
 * (integer) atomics on the device, where the floating-point partials forbid atomics.
 *
 * Quantiles.  For a probability q and a dimension of m finite values: h = (double)(m - 1) * q (rounded once), lo = floor(h),
 * g = h - lo, hi = min(lo + 1, m - 1) - numpy's "linear" virtual index.  With x_lo and x_hi the order statistics of ranks lo and hi
 * (0-based, ascending), the quantile is x_lo where g = 0 and fma(g, x_hi - x_lo, x_lo) otherwise (x_hi - x_lo rounded once; it
 * overflows only for values more than DBL_MAX apart).  m = 0: NaN.
 */
#ifndef RMHMC_QUANT_H
#define RMHMC_QUANT_H

#include "rmhmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define RMHMC_QUANT_MAX_K 16 /* most targets per dimension of one histogram call */
#define RMHMC_QUANT_MAX_Q 8  /* most probabilities of one plan: two targets each */

/* The histogram partial of round `round` of samples_dev [n][S][P] (device memory) -> hist_dev [Kh][P][256] (device memory).  prefix:
 * host, [K][P], NULL in round 0 (K is then checked and otherwise unused).  Stream and synchronisation as rmhmc_ess_dev (rmhmc_out.h):
 * the samples must be complete before the call, the library's stream is idle on return.  The chain state of the context is not touched.
 * Invalid arguments are refused on the host before any device work, hist_dev untouched: RMHMC_ERR_INVALID for a NULL pointer (prefix in
 * a round after 0 included), n, S or P < 1, round outside 0 .. 7 or K outside 1 .. 16. */
int rmhmc_quant_hist_dev(rmhmc_ctx *ctx, const double *samples_dev, int64_t n, int64_t S, int32_t P, int32_t round,
                         const uint64_t *prefix, int32_t K, double *hist_dev);

/* Host only, no context: the targets of Q probabilities.  m [P]: the finite values per dimension; rank [2Q][P]: rows 2j and 2j+1 are
 * lo and hi of probs[j], -1 where m_d = 0; frac [Q][P]: g (0 where m_d = 0).  RMHMC_ERR_INVALID for a NULL pointer, P < 1, Q outside
 * 1 .. 8, a negative m, or a probability outside [0, 1] or NaN; nothing is written then. */
int rmhmc_quant_plan(const int64_t *m, const double *probs, int32_t Q, int32_t P, int64_t *rank, double *frac);

/* Host only, no context: one round of the select.  Merges the k_parts histograms of round `round` (host pointers, [Kh][P][256] each) in
 * the order given; per target picks the first bin whose cumulative count exceeds the remaining rank, writes the bin into prefix[K][P]
 * and subtracts the counts below the bin from rank[K][P].  Targets of rank -1 are carried through unchanged.  RMHMC_ERR_INVALID, and
 * nothing written, for a NULL pointer, k_parts or P < 1, K outside 1 .. 16, round outside 0 .. 7, an entry that is not a count, and
 * for a histogram whose total for a target is not the count of the bin chosen in the previous round (partials of different samples, a
 * skipped round), in round 0: whose total is not above the rank.  RMHMC_ERR_NOMEM. */
int rmhmc_quant_step(const double *const *hists, int32_t k_parts, int32_t P, int32_t K, int32_t round, uint64_t *prefix, int64_t *rank);

/* Host only, no context: prefix [2Q][P] after round 7, frac [Q][P] and m [P] of the plan -> quant [Q][P].  RMHMC_ERR_INVALID for a
 * NULL pointer, P < 1 or Q outside 1 .. 8. */
int rmhmc_quant_finish(const uint64_t *prefix, const double *frac, const int64_t *m, int32_t Q, int32_t P, double *quant);

/* All eight rounds on one shard: quant [Q][P] and draws_used [P] (= m; may be NULL), both host.  Equal bit for bit to round 0 of
 * rmhmc_quant_hist_dev, rmhmc_quant_plan on its totals, rmhmc_quant_step, rounds 1 .. 7 with K = 2Q each followed by its step, and
 * rmhmc_quant_finish.  Stream, synchronisation and refusals as those calls. */
int rmhmc_quant_dev(rmhmc_ctx *ctx, const double *samples_dev, int64_t n, int64_t S, int32_t P, const double *probs, int32_t Q,
                    double *quant, int64_t *draws_used);

#ifdef __cplusplus
}
#endif

#endif /* RMHMC_QUANT_H */
