// adapt.h — the host half of the warm-up of the fixed-metric HMC sampler (include/rmhmc_adapt.h): the shape of a covariance partial
// and the row blocks the kernels of adapt.hip.h work on, the merge of two partials and the finish, the regularised mass matrix, and
// dual averaging of the step size.  No HIP header: plain C++17, so a host compiler alone builds it (tests/helpers/adapt_probe.cpp)
// and the library calls the same code (rmhmc_cov_finish, rmhmc_adapt_mass, rmhmc_adapt_init, rmhmc_adapt_step, rmhmc_phmc_warmup).
//
// A partial of P is double[(2 + P) * P], rows of length P, about the rows used (a row with a non-finite entry is not used):
//   row 0      m, the number of rows used (an exact integer, in every entry)
//   row 1      their mean
//   row 2 + i  row i of C = sum over them of (x - mean)(x - mean)', full and exactly symmetric
#pragma once
#include "../../include/rmhmc.h"
#include "mass.h"

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <new>
#include <vector>

// ---- shape constants of adapt.hip.h ----------------------------------------------------------------------------------------------------
#define COV_MAX_P 256
#define COV_ROWS 256                       // the smallest row block: a constant, so the split of N rows depends on (N, P) alone
#define COV_MAX_BLOCKS 1024                // row blocks of either pass
#define COV_SCRATCH_BYTES (4 << 20)        // bound of the [nblocks][P][P] scratch of the second pass: 8 blocks at P = 256

// row blocks of the second pass and the rows of one (a multiple of 4, the rows of one MFMA): as many blocks of at least COV_ROWS rows
// as the scratch bound allows
inline int64_t cov_max_blocks(int32_t P) {
  const int64_t b = (int64_t)COV_SCRATCH_BYTES / ((int64_t)8 * P * P);
  return b < 1 ? 1 : b > COV_MAX_BLOCKS ? COV_MAX_BLOCKS : b;
}
inline void cov_plan(int64_t N, int32_t P, int64_t* nblocks, int64_t* rows_per_block) {
  int64_t nb = (N + COV_ROWS - 1) / COV_ROWS;
  const int64_t mb = cov_max_blocks(P);
  if (nb > mb) nb = mb;
  const int64_t rpb = ((N + nb - 1) / nb + 3) / 4 * 4;
  *rows_per_block = rpb;
  *nblocks = (N + rpb - 1) / rpb;
}
// row blocks of the first pass (column sums): at least COV_ROWS rows each, at most COV_MAX_BLOCKS
inline void cov_plan_sums(int64_t N, int64_t* nblocks, int64_t* rows_per_block) {
  int64_t nb = (N + COV_ROWS - 1) / COV_ROWS;
  if (nb > COV_MAX_BLOCKS) nb = COV_MAX_BLOCKS;
  *rows_per_block = (N + nb - 1) / nb;
  *nblocks = (N + *rows_per_block - 1) / *rows_per_block;
}

// ---- merge and finish ------------------------------------------------------------------------------------------------------------------
// a <- a merged with b (both of P) by Chan's update.  A partial with m = 0 is the identity.
inline void cov_merge(double* a, const double* b, int32_t P) {
  const size_t p = (size_t)P;
  const double ma = a[0], mb = b[0];
  if (mb == 0.0) return;
  if (ma == 0.0) {
    for (size_t i = 0; i < (2 + p) * p; ++i) a[i] = b[i];
    return;
  }
  const double m = ma + mb, w = ma * mb / m;
  std::vector<double> delta(p);
  for (size_t d = 0; d < p; ++d) delta[d] = b[p + d] - a[p + d];
  for (size_t d = 0; d < p; ++d) {
    a[d] = m;
    a[p + d] = a[p + d] + delta[d] * mb / m;
  }
  for (size_t i = 0; i < p; ++i)
    for (size_t j = 0; j <= i; ++j) {
      const double c = a[(2 + i) * p + j] + b[(2 + i) * p + j] + delta[i] * delta[j] * w;
      a[(2 + i) * p + j] = a[(2 + j) * p + i] = c;
    }
}

// rmhmc_cov_finish (include/rmhmc_adapt.h): merges the k partials in the order given into `merged` (or a buffer of its own) and
// finishes: mean = row 1, cov = C / (m - 1), NaN for m < 2.  Returns RMHMC_OK, RMHMC_ERR_INVALID, RMHMC_ERR_NOMEM.
inline int cov_finish(const double* const* partials, int32_t k, int32_t P, double* merged, double* mean, double* cov, int64_t* rows_used) {
  if (!partials || k < 1 || P < 1) return RMHMC_ERR_INVALID;
  for (int32_t i = 0; i < k; ++i)
    if (!partials[i]) return RMHMC_ERR_INVALID;
  const size_t p = (size_t)P, len = (2 + p) * p;
  double* own = nullptr;
  if (!merged) {
    own = new (std::nothrow) double[len];
    if (!own) return RMHMC_ERR_NOMEM;
    merged = own;
  }
  for (size_t i = 0; i < len; ++i) merged[i] = 0.0;
  for (int32_t i = 0; i < k; ++i) cov_merge(merged, partials[i], P);
  const double m = merged[0];
  if (mean)
    for (size_t d = 0; d < p; ++d) mean[d] = merged[p + d];
  if (cov)
    for (size_t i = 0; i < p * p; ++i) cov[i] = m >= 2.0 ? merged[2 * p + i] / (m - 1.0) : NAN;
  if (rows_used) *rows_used = (int64_t)m;
  delete[] own;
  return RMHMC_OK;
}

// ---- regularised mass ------------------------------------------------------------------------------------------------------------------
// Sigma_reg = m / (m + 5) cov + 1e-3 * 5 / (m + 5) I (the shrinkage of Stan's warm-up: cited, not measured here); Mass = Sigma_reg^-1 is
// the Minv image mass_images makes of Sigma_reg.  mass [P][P] is written only on success; *why says what was refused.
inline int adapt_mass(const double* cov, int64_t m, int32_t P, double* mass, const char** why) {
  *why = "";
  if (!cov || !mass || P < 1) { *why = "adapt_mass: NULL pointer or P < 1"; return RMHMC_ERR_INVALID; }
  if (m < 2) { *why = "adapt_mass: fewer than 2 rows"; return RMHMC_ERR_INVALID; }
  const size_t p = (size_t)P;
  const double md = (double)m, wc = md / (md + 5.0), wi = 1e-3 * (5.0 / (md + 5.0));
  std::vector<double> sig(p * p), Lm, Minv;
  for (size_t i = 0; i < p; ++i)
    for (size_t j = 0; j < p; ++j) {
      const double v = wc * cov[i * p + j] + (i == j ? wi : 0.0);
      if (!std::isfinite(v)) { *why = "adapt_mass: the covariance is not finite"; return RMHMC_ERR_INVALID; }
      sig[i * p + j] = v;
    }
  if (mass_images(sig.data(), P, P, Lm, Minv, why) != RMHMC_OK) return RMHMC_ERR_INVALID;
  for (size_t i = 0; i < p * p; ++i) mass[i] = Minv[i];
  return RMHMC_OK;
}

// ---- dual averaging of log eps (Hoffman & Gelman 2014, section 3.2) ---------------------------------------------------------------------
// state = (t, Hbar, log epsbar, mu); a (re)start at eps has mu = log(factor eps): the paper's factor 10 at the start of a warm-up, 1 at
// its restarts after a mass update (include/rmhmc_adapt.h says why)
#define ADAPT_FACTOR_START 10.0
#define ADAPT_FACTOR_RESTART 1.0
inline int adapt_init(double state[4], double eps, double factor) {
  if (!state || !std::isfinite(eps) || !(eps > 0.0) || !std::isfinite(factor) || !(factor > 0.0)) return RMHMC_ERR_INVALID;
  state[0] = 0.0;
  state[1] = 0.0;
  state[2] = 0.0;
  state[3] = log(factor * eps);
  return RMHMC_OK;
}

inline int adapt_step(double state[4], double accept, double delta, double gamma, double t0, double kappa, double* eps_next, double* eps_bar) {
  if (!state || !std::isfinite(accept)) return RMHMC_ERR_INVALID;
  const double t = state[0] + 1.0;
  const double Hbar = (1.0 - 1.0 / (t + t0)) * state[1] + (delta - accept) / (t + t0);
  const double leps = state[3] - sqrt(t) / gamma * Hbar;
  const double eta = pow(t, -kappa);
  const double lbar = eta * leps + (1.0 - eta) * state[2];
  const double e = exp(leps), eb = exp(lbar);
  if (!std::isfinite(e) || !(e > 0.0) || !std::isfinite(eb) || !(eb > 0.0)) return RMHMC_ERR_INVALID;
  state[0] = t;
  state[1] = Hbar;
  state[2] = lbar;
  if (eps_next) *eps_next = e;
  if (eps_bar) *eps_bar = eb;
  return RMHMC_OK;
}

// ---- the schedule ----------------------------------------------------------------------------------------------------------------------
// W = warmup / window windows of `window` iterations: the first max(1, round(0.15 W)) and the last max(1, round(0.1 W)) of kind 0 (step
// size only), the rest of kind 1 (step size, then mass); halves round up.  Returns W, or 0 where W < 3 or window < 1 (refused);
// win_len / win_kind [W] are filled where given.
inline int64_t adapt_schedule(int64_t warmup, int64_t window, int64_t* win_len, int32_t* win_kind) {
  if (window < 1 || warmup / window < 3) return 0;
  const int64_t W = warmup / window;
  int64_t head = (15 * W + 50) / 100, tail = (10 * W + 50) / 100;
  if (head < 1) head = 1;
  if (tail < 1) tail = 1;
  for (int64_t w = 0; w < W; ++w) {
    if (win_len) win_len[w] = window;
    if (win_kind) win_kind[w] = (w < head || w >= W - tail) ? 0 : 1;
  }
  return W;
}

// the acceptance statistic of a window: accepted proposals of all chains over n K transitions
inline double adapt_accept(const int64_t* accepted, int64_t n, int64_t K) {
  int64_t s = 0;
  for (int64_t c = 0; c < n; ++c) s += accepted[c];
  return (double)s / ((double)n * (double)K);
}
