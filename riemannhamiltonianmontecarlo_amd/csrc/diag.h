// diag.h — the host half of the cross-chain diagnostics (include/rmhmc_diag.h): the shape of a partial, the tile the kernel of
// diag.hip.h works on, the merge of two partials and the finish (split R-hat, pooled ESS).  No HIP header: plain C++17, so a host
// compiler alone builds it (tests/helpers/diag_probe.cpp) and the library calls the same code (rmhmc_diag_finish).
//
// A partial of (H, T, P) is double[(4 + T) * P], rows of length P, about the series used in dimension d (a series = one half of a chain
// in one dimension; one with a non-finite value is not used):
//   row 0      m      number of series used (an exact integer)
//   row 1      mean of their means
//   row 2      M2 = sum over them of (mean_j - row 1)^2
//   row 3      sum of their sample variances s2_j = acov_j(0) H / (H - 1)
//   row 4 + t  sum of their biased autocovariances acov_j(t) = (1/H) sum_s (x_s - mean_j)(x_{s+t} - mean_j),  t = 0 .. T-1
#pragma once
#include "../../include/rmhmc.h"

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <new>

// ---- shape constants of diag.hip.h -----------------------------------------------------------------------------------------------------
#define DIAG_CHAINS 32        // chains of one workgroup of k_diag_acov: a constant, so a block's sum never depends on the grid
#define DIAG_THREADS 256
#define DIAG_R 16             // lags a thread holds in registers
#define DIAG_MAX_TW 64        // widest dimension tile
#define DIAG_LDS_BYTES (160 * 1024)
#define DIAG_LDS_SHARED (80 * 1024)   // a tile of at most this leaves room for a second workgroup on the CU
#define DIAG_NQ 4             // sets of DIAG_R lags a thread holds when one set per thread does not cover T

// rows of the LDS image of one half-series tile: H rounded up to the 16-row step of the lag loop, plus the 32 zero rows its window
// reads past the end; one pad row after every 16 (threads of different lag groups then start in different banks)
inline int64_t diag_lds_rows(int64_t H) {
  const int64_t rows = (H + 15) / 16 * 16 + 32;
  return rows + rows / 16;
}
// LDS bytes of a workgroup: the tile, then one double and one flag per thread for the column sums
inline int64_t diag_lds_bytes(int64_t H, int tw) { return (diag_lds_rows(H) * tw + DIAG_THREADS) * 8 + DIAG_THREADS * 4; }
// dimension-tile width: the largest power of two <= 64 that is not wider than P needs and whose tile leaves room for a second
// workgroup on the CU, or else fits the LDS at all; 0: none fits
inline int diag_tile_width(int64_t H, int32_t P) {
  int tw = DIAG_MAX_TW;
  while (tw > 1 && tw / 2 >= P) tw /= 2;
  while (tw > 1 && diag_lds_bytes(H, tw) > DIAG_LDS_SHARED) tw /= 2;
  return diag_lds_bytes(H, tw) > DIAG_LDS_BYTES ? 0 : tw;
}
// lags one workgroup covers with one set of DIAG_R lags per thread, and the sets per thread for T lags.  DIAG_NQ sets cover every
// T <= H: a width tw > 1 is chosen only where (17/16 (H + 47) tw + 256) 8 + 1024 <= 81920, i.e. H tw < 9500, and 64 * 256 / tw lags
// are then more than 1.7 H; at tw = 1 they are 16384 against H <= 10000.
inline int64_t diag_lags_per_block(int tw) { return (int64_t)(DIAG_THREADS / tw) * DIAG_R; }
inline int diag_lag_sets(int64_t T, int tw) { return T > diag_lags_per_block(tw) ? DIAG_NQ : 1; }

// ---- merge and finish ------------------------------------------------------------------------------------------------------------------
// a <- a merged with b (both of (T, P)): rows 0, 3, 4.. add; rows 1 and 2 by Chan's update.  A partial with m = 0 is the identity.
inline void diag_merge(double* a, const double* b, int64_t T, int32_t P) {
  for (int32_t d = 0; d < P; ++d) {
    const double ma = a[d], mb = b[d];
    if (mb == 0.0) continue;
    if (ma == 0.0) {
      for (int64_t r = 0; r < 4 + T; ++r) a[r * P + d] = b[r * P + d];
      continue;
    }
    const double m = ma + mb, delta = b[P + d] - a[P + d];
    a[d] = m;
    a[P + d] = a[P + d] + delta * mb / m;
    a[2 * P + d] = a[2 * P + d] + b[2 * P + d] + delta * delta * ma * mb / m;
    for (int64_t r = 3; r < 4 + T; ++r) a[r * P + d] += b[r * P + d];
  }
}

// One dimension of a merged partial (column d, stride P) -> split R-hat, pooled ESS and the number of Geyer pairs summed.
//   W = row3 / m, B/H = M2 / (m - 1), var+ = W (H-1)/H + B/H, rhat = sqrt(var+ / W)
//   rho_0 = 1, rho_t = 1 - (W - row[4+t] / m) / var+;  Gamma_k = rho_2k + rho_2k+1, replaced by its running minimum, summed while > 0
//   and 2k+1 < T (the rule of k_ess);  tau = max(1, -1 + 2 sum),  ess = m H / tau.
// 2 pairs + 1 >= T: the lags ran out before the sequence ended, and ess is an upper bound (always so when the chains disagree: rho_t
// then tends to 1 - W / var+ > 0).  m < 2 or W not > 0: NaN, NaN, 0.
inline void diag_finish_dim(const double* col, int64_t H, int64_t T, int32_t P, double* rhat, double* ess, int64_t* pairs) {
  const double m = col[0];
  const double W = m > 0.0 ? col[3 * (size_t)P] / m : 0.0;
  *rhat = *ess = NAN;
  *pairs = 0;
  if (!(m >= 2.0) || !(W > 0.0)) return;
  const double BH = col[2 * (size_t)P] / (m - 1.0);
  const double varp = W * (double)(H - 1) / (double)H + BH;
  *rhat = sqrt(varp / W);
  double prev = INFINITY, sum = 0.0;
  int64_t k = 0;
  for (; 2 * k + 1 < T; ++k) {
    const double r0 = k == 0 ? 1.0 : 1.0 - (W - col[(4 + 2 * k) * (size_t)P] / m) / varp;
    const double r1 = 1.0 - (W - col[(4 + 2 * k + 1) * (size_t)P] / m) / varp;
    double g = r0 + r1;
    if (g > prev) g = prev;
    if (!(g > 0.0)) break;
    sum += g;
    prev = g;
  }
  double tau = -1.0 + 2.0 * sum;
  if (tau < 1.0) tau = 1.0;
  *ess = m * (double)H / tau;
  *pairs = k;
}

// rmhmc_diag_finish (include/rmhmc_diag.h): merges the k partials in the order given into `merged` (or a buffer of its own) and finishes
// every dimension; `merged` may not be one of the partials.  Returns RMHMC_OK, RMHMC_ERR_INVALID for an argument out of range, RMHMC_ERR_NOMEM.
inline int diag_finish(const double* const* partials, int32_t k, int64_t H, int64_t T, int32_t P, double* merged, double* rhat, double* ess,
                       int64_t* pairs, int64_t* chains_used) {
  if (!partials || k < 1 || H < 2 || T < 2 || T > H || P < 1) return RMHMC_ERR_INVALID;
  for (int32_t i = 0; i < k; ++i)
    if (!partials[i]) return RMHMC_ERR_INVALID;
  const size_t len = (size_t)(4 + T) * (size_t)P;
  double* own = nullptr;
  if (!merged) {
    own = new (std::nothrow) double[len];
    if (!own) return RMHMC_ERR_NOMEM;
    merged = own;
  }
  for (size_t i = 0; i < len; ++i) merged[i] = 0.0;
  for (int32_t i = 0; i < k; ++i) diag_merge(merged, partials[i], T, P);
  for (int32_t d = 0; d < P; ++d) {
    double r, e;
    int64_t np;
    diag_finish_dim(merged + d, H, T, P, &r, &e, &np);
    if (rhat) rhat[d] = r;
    if (ess) ess[d] = e;
    if (pairs) pairs[d] = np;
    if (chains_used) chains_used[d] = (int64_t)merged[d];
  }
  delete[] own;
  return RMHMC_OK;
}
