// loo.h — the host half of leave-one-out cross-validation (include/rmhmc_loo.h): the shape of the partials, the merge of two moments
// partials, the tail length, the finish, the host checks, and the plan of the kernels of loo.hip.h (row blocks, scratch) as functions
// of (N, C, D).  No HIP header: plain C++17, so a host compiler alone builds it (tests/helpers/loo_probe.cpp) and the library calls the
// same code (rmhmc_loo_plan, rmhmc_loo_finish, rmhmc_loo_dev).
#pragma once
#include "../../include/rmhmc.h"

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <new>

// ---- shape constants of loo.hip.h -----------------------------------------------------------------------------------------------------------
#define LOO_MAX_D 256
#define LOO_MAX_COLS 64          // columns of one device call: four wavefronts of 16 (the A operand), and the widest tile of the select
#define LOO_MAX_TAIL 16384       // doubles of a column's tail in LDS
#define LOO_DRAWS 256            // draws of a workgroup of the log-likelihood kernel
#define LOO_ROW_LANES 4          // row lanes of a column in a reduction workgroup: 256 threads = LOO_ROW_LANES x LOO_MAX_COLS, whatever C is
#define LOO_BLOCK_ROWS 4096      // rows of a reduction block while LOO_MAX_BLOCKS allows
#define LOO_MAX_BLOCKS 1024      // blocks of a reduction
#define LOO_REC 4                // values of a block's record per column
#define LOO_FIT_THREADS 256
#define LOO_MAX_G 160            // 30 + floor(sqrt(LOO_MAX_TAIL)) = 158 candidates of the fit
#define LOO_LL_BYTES ((int64_t)1 << 31)   // bound of an ll block of rmhmc_loo_dev

struct loo_plan_t {
  int64_t lblocks;          // workgroups of the log-likelihood kernel, LOO_DRAWS draws each
  int64_t vblocks;          // draw blocks of the validity pass (k_pred_valid)
  int64_t draws_per_vblock;
  int64_t rblocks;          // row blocks of a reduction over ll: a function of N alone, so that a column's sums do not depend on C
  int64_t rows_per_block;   // a multiple of LOO_ROW_LANES
  int32_t ksteps;           // MFMA steps the log-likelihood kernel is compiled for (as pred_ksteps)
};

inline int32_t loo_ksteps(int32_t D) { return D <= 16 ? 4 : (D + 31) / 32 * 8; }

inline loo_plan_t loo_kernel_plan(int64_t N, int32_t D) {
  loo_plan_t p;
  p.lblocks = (N + LOO_DRAWS - 1) / LOO_DRAWS;
  int64_t vb = (N + LOO_DRAWS - 1) / LOO_DRAWS;
  if (vb > LOO_MAX_BLOCKS) vb = LOO_MAX_BLOCKS;
  p.draws_per_vblock = (N + vb - 1) / vb;
  p.vblocks = (N + p.draws_per_vblock - 1) / p.draws_per_vblock;
  int64_t rb = (N + LOO_BLOCK_ROWS - 1) / LOO_BLOCK_ROWS;
  if (rb > LOO_MAX_BLOCKS) rb = LOO_MAX_BLOCKS;
  p.rows_per_block = ((N + rb - 1) / rb + LOO_ROW_LANES - 1) / LOO_ROW_LANES * LOO_ROW_LANES;
  p.rblocks = (N + p.rows_per_block - 1) / p.rows_per_block;
  p.ksteps = loo_ksteps(D);
  return p;
}

// cols_per_block of rmhmc_loo_dev where the caller leaves it to the library: the largest power of two <= 64 whose ll block stays
// within LOO_LL_BYTES, at least 1
inline int32_t loo_cols_per_block(int64_t N) {
  int32_t c = LOO_MAX_COLS;
  while (c > 1 && (N > LOO_LL_BYTES / 8 / c)) c /= 2;
  return c;
}

// ---- the host checks of the device calls: nullptr, or what is refused -------------------------------------------------------------------------
inline const char* loo_check_rows(const double* x, const double* t, int64_t C, int32_t D) {
  for (int64_t i = 0; i < C * (int64_t)D; ++i)
    if (!std::isfinite(x[i])) return "an entry of x is not finite";
  for (int64_t c = 0; c < C; ++c)
    if (!(t[c] == 0.0 || t[c] == 1.0)) return "an entry of t is neither 0 nor 1";
  return nullptr;
}
inline const char* loo_check_tails(const int64_t* tail_len, int64_t C, int64_t stride) {
  if (stride < 1) return "stride >= 1";
  for (int64_t c = 0; c < C; ++c)
    if (tail_len[c] < 0 || tail_len[c] > stride || tail_len[c] > LOO_MAX_TAIL) return "a tail length outside 0 .. min(stride, 16384)";
  return nullptr;
}

// ---- tail length ----------------------------------------------------------------------------------------------------------------------------
// M = min(floor(m / 5), r), r the smallest integer with r^2 >= 9 m.  m >= 0 and below 2^59.
inline int64_t loo_tail_len(int64_t m) {
  const int64_t nine = 9 * m;
  int64_t r = (int64_t)sqrt((double)nine);
  while (r * r < nine) ++r;
  while (r > 0 && (r - 1) * (r - 1) >= nine) --r;
  const int64_t fifth = m / 5;
  return fifth < r ? fifth : r;
}

inline int loo_plan(const int64_t* m, int32_t C, int64_t* tail_len, int64_t* rank) {
  if (!m || !tail_len || !rank || C < 1) return RMHMC_ERR_INVALID;
  for (int32_t c = 0; c < C; ++c)
    if (m[c] < 0 || m[c] > ((int64_t)1 << 59)) return RMHMC_ERR_INVALID;
  for (int32_t c = 0; c < C; ++c)
    if (loo_tail_len(m[c]) > LOO_MAX_TAIL) return RMHMC_ERR_UNSUPPORTED;
  for (int32_t c = 0; c < C; ++c) {
    const int64_t M = loo_tail_len(m[c]);
    tail_len[c] = M;
    rank[c] = M < 5 ? -1 : M;
  }
  return RMHMC_OK;
}

// ---- merge and finish -----------------------------------------------------------------------------------------------------------------------
// the partial of no draws: m = mean = M2 = SQ = 0, lmin = +inf
inline void loo_identity(double* a, int64_t C) {
  for (int64_t i = 0; i < 4 * C; ++i) a[i] = 0.0;
  for (int64_t i = 4 * C; i < 5 * C; ++i) a[i] = INFINITY;
}

// a <- a merged with b (both of C columns), column by column; a column of m = 0 on either side changes no bit of the other
inline void loo_merge(double* a, const double* b, int64_t C) {
  const size_t n = (size_t)C;
  for (size_t c = 0; c < n; ++c) {
    const double mb = b[c];
    if (mb == 0.0) continue;
    const double ma = a[c];
    if (ma == 0.0) {
      for (int q = 0; q < 5; ++q) a[q * n + c] = b[q * n + c];
      continue;
    }
    const double m = ma + mb, delta = b[n + c] - a[n + c];
    a[c] = m;
    a[n + c] = a[n + c] + delta * (mb / m);
    a[2 * n + c] = (a[2 * n + c] + b[2 * n + c]) + delta * delta * (ma * (mb / m));
    a[3 * n + c] += b[3 * n + c];
    if (b[4 * n + c] < a[4 * n + c]) a[4 * n + c] = b[4 * n + c];
  }
}

// sum in index order and sqrt(C var), var the sample variance (C - 1) about the mean of that sum; NaN for C < 2
inline void loo_total_se(const double* v, size_t C, double* total, double* se) {
  double s = 0.0;
  for (size_t c = 0; c < C; ++c) s += v[c];
  *total = s;
  *se = NAN;
  if (C < 2) return;
  const double mean = s / (double)C;
  double q = 0.0;
  for (size_t c = 0; c < C; ++c) q += (v[c] - mean) * (v[c] - mean);
  *se = sqrt((double)C * (q / (double)(C - 1)));
}

// rmhmc_loo_finish (include/rmhmc_loo.h).  Returns RMHMC_OK, RMHMC_ERR_INVALID, RMHMC_ERR_NOMEM.
inline int loo_finish(const double* const* partials, int32_t k, int64_t C, const double* fit, const double* body, double* merged,
                      double* elpd_loo, double* p_loo, double* pareto_k, double* lppd, double* p_waic, double* elpd_waic, double* totals,
                      int64_t* k_counts, int64_t* draws_used) {
  if (!partials || k < 1 || C < 1 || (fit == nullptr) != (body == nullptr)) return RMHMC_ERR_INVALID;
  for (int32_t i = 0; i < k; ++i)
    if (!partials[i]) return RMHMC_ERR_INVALID;
  const size_t n = (size_t)C;
  double* work = new (std::nothrow) double[8 * n];   // the merged partial, elpd_loo, p_loo, elpd_waic
  if (!work) return RMHMC_ERR_NOMEM;
  double *mg = work, *el = work + 5 * n, *pl = work + 6 * n, *ew = work + 7 * n;
  loo_identity(mg, C);
  for (int32_t i = 0; i < k; ++i) loo_merge(mg, partials[i], C);
  int64_t mid = 0, high = 0;
  for (size_t c = 0; c < n; ++c) {
    const double m = mg[c];
    double lp = NAN, pw = NAN, e = NAN, kh = NAN;
    if (m > 0.0) {
      lp = log(mg[3 * n + c] / m);
      if (m >= 2.0) pw = mg[2 * n + c] / (m - 1.0);
      if (fit) {
        kh = fit[c];
        e = log(fit[3 * n + c] + body[n + c]) - log(fit[2 * n + c] + body[c]);
      }
    }
    el[c] = e;
    pl[c] = lp - e;
    ew[c] = lp - pw;
    if (kh > 0.7) ++high;
    else if (kh > 0.5) ++mid;
    if (pareto_k) pareto_k[c] = kh;
    if (lppd) lppd[c] = lp;
    if (p_waic) p_waic[c] = pw;
    if (draws_used) draws_used[c] = (int64_t)m;
  }
  if (totals) {
    double unused;
    loo_total_se(el, n, &totals[0], &totals[1]);
    loo_total_se(pl, n, &totals[2], &unused);
    loo_total_se(ew, n, &totals[3], &totals[4]);
    double s = 0.0;
    for (size_t c = 0; c < n; ++c) s += mg[c] >= 2.0 ? mg[2 * n + c] / (mg[c] - 1.0) : NAN;
    totals[5] = s;
  }
  if (k_counts) { k_counts[0] = mid; k_counts[1] = high; }
  for (size_t c = 0; c < n; ++c) {
    if (elpd_loo) elpd_loo[c] = el[c];
    if (p_loo) p_loo[c] = pl[c];
    if (elpd_waic) elpd_waic[c] = ew[c];
  }
  if (merged)
    for (size_t i = 0; i < 5 * n; ++i) merged[i] = mg[i];
  delete[] work;
  return RMHMC_OK;
}
