// ais.h — the host half of annealed importance sampling (include/rmhmc_ais.h): the blocks the weight kernels of ais.hip.h work on, the
// merge of two weight partials and the finish, the temperature ladders and the stage_mass pattern, the argument checks of
// rmhmc_ais_run, and the mass matrix of a stage.  No HIP header: plain C++17, so a host compiler alone builds it
// (tests/helpers/ais_probe.cpp) and the library calls the same code (rmhmc_ais_finish, rmhmc_ais_run).
//
// A partial is double[5] = (m, n_nan, a, S1, S2): see include/rmhmc_ais.h.
#pragma once
#include "../../include/rmhmc.h"
#include "mass.h"

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

// ---- blocks of k_ais_max / k_ais_sums: at least AIS_ROWS entries each, a multiple of it, at most AIS_MAX_BLOCKS: n alone decides ----
#define AIS_ROWS 256
#define AIS_MAX_BLOCKS 1024
inline void ais_plan(int64_t n, int64_t* nblocks, int64_t* per_block) {
  int64_t nb = (n + AIS_ROWS - 1) / AIS_ROWS;
  if (nb > AIS_MAX_BLOCKS) nb = AIS_MAX_BLOCKS;
  if (nb < 1) nb = 1;
  const int64_t pb = ((n + nb - 1) / nb + AIS_ROWS - 1) / AIS_ROWS * AIS_ROWS;
  *per_block = pb < AIS_ROWS ? AIS_ROWS : pb;
  *nblocks = n < 1 ? 1 : (n + *per_block - 1) / *per_block;
}

// ---- merge and finish ------------------------------------------------------------------------------------------------------------------
inline void ais_empty(double acc[5]) {
  acc[0] = 0.0; acc[1] = 0.0; acc[2] = -HUGE_VAL; acc[3] = 0.0; acc[4] = 0.0;
}
// acc <- acc merged with p.  A partial with m = 0 is the identity (its n_nan is still counted).
inline void ais_merge(double acc[5], const double p[5]) {
  acc[1] += p[1];
  if (p[0] == 0.0) return;
  if (acc[0] == 0.0) {
    acc[0] = p[0]; acc[2] = p[2]; acc[3] = p[3]; acc[4] = p[4];
    return;
  }
  const double a = acc[2] > p[2] ? acc[2] : p[2];
  acc[0] += p[0];
  if (a == -HUGE_VAL) {  // weights of zero on both sides
    acc[2] = a; acc[3] = 0.0; acc[4] = 0.0;
    return;
  }
  const double da = acc[2] - a, dp = p[2] - a;  // (one of them is 0: its factor is exactly 1)
  acc[3] = acc[3] * exp(da) + p[3] * exp(dp);
  acc[4] = acc[4] * exp(2.0 * da) + p[4] * exp(2.0 * dp);
  acc[2] = a;
}
// every output may be nullptr
inline int ais_finish(const double* const* partials, int32_t k, double* merged, double* log_mean_w, double* se, double* weight_ess,
                      int64_t* m_out, int64_t* n_nan_out) {
  if (k < 1 || !partials) return RMHMC_ERR_INVALID;
  for (int32_t i = 0; i < k; ++i)
    if (!partials[i]) return RMHMC_ERR_INVALID;
  double acc[5];
  ais_empty(acc);
  for (int32_t i = 0; i < k; ++i) ais_merge(acc, partials[i]);
  const double m = acc[0], a = acc[2], S1 = acc[3], S2 = acc[4];
  double lm = NAN, s = NAN, ess = NAN;
  if (m > 0.0) {
    if (S1 > 0.0) {
      lm = a + log(S1 / m);
      ess = S1 * S1 / S2;
      if (m >= 2.0) {
        const double v = (m * S2 / (S1 * S1) - 1.0) / (m - 1.0);
        s = sqrt(v > 0.0 ? v : v == v ? 0.0 : v);  // (equal weights: the bracket is 0 up to rounding)
      }
    } else if (S1 == 0.0) {
      lm = -HUGE_VAL;
    }
  }
  if (merged) for (int i = 0; i < 5; ++i) merged[i] = acc[i];
  if (log_mean_w) *log_mean_w = lm;
  if (se) *se = s;
  if (weight_ess) *weight_ess = ess;
  if (m_out) *m_out = (int64_t)m;
  if (n_nan_out) *n_nan_out = (int64_t)acc[1];
  return RMHMC_OK;
}

// ---- ladders and the stage_mass pattern ----------------------------------------------------------------------------------------------------
// power ladder beta_k = ((k + 1) / T)^q, k = 0 .. T - 1 (the last is exactly 1).  RMHMC_ERR_INVALID for T < 1 or a q that is not finite
// and > 0.
inline int ais_ladder_power(int64_t T, double q, double* beta) {
  if (T < 1 || !beta || !isfinite(q) || !(q > 0.0)) return RMHMC_ERR_INVALID;
  for (int64_t k = 0; k < T; ++k) beta[k] = k == T - 1 ? 1.0 : pow((double)(k + 1) / (double)T, q);
  return RMHMC_OK;
}
// log-spaced ladder beta_k = beta_min^(1 - (k + 1) / T): from just above beta_min to exactly 1.  RMHMC_ERR_INVALID for T < 1 or a beta_min
// outside (0, 1).
inline int ais_ladder_log(int64_t T, double beta_min, double* beta) {
  if (T < 1 || !beta || !(beta_min > 0.0) || !(beta_min < 1.0)) return RMHMC_ERR_INVALID;
  const double l = log(beta_min);
  for (int64_t k = 0; k < T; ++k) beta[k] = k == T - 1 ? 1.0 : exp(l * (1.0 - (double)(k + 1) / (double)T));
  return RMHMC_OK;
}
// a mass update every mass_every stages, and in the first and the last
inline int ais_stage_mass(int64_t T, int64_t mass_every, int32_t* stage_mass) {
  if (T < 1 || mass_every < 1 || !stage_mass) return RMHMC_ERR_INVALID;
  for (int64_t k = 0; k < T; ++k) stage_mass[k] = (k % mass_every == 0 || k == T - 1) ? 1 : 0;
  return RMHMC_OK;
}

// ---- rmhmc_ais_run: its refusals (nullptr: none) and the mass of a stage --------------------------------------------------------------------
inline bool ais_beta_ok(double b) { return isfinite(b) && b >= 0.0; }
inline const char* ais_check_run(bool have_theta0, double beta0, int32_t T, const double* beta, const int64_t* stage_len,
                                 const int32_t* stage_mass, bool have_H, int32_t L) {
  if (T < 1 || !beta || !stage_len) return "need T >= 1 stages, beta and stage_len";
  if (L < 1) return "need L >= 1";
  if (!ais_beta_ok(beta0)) return "beta0 must be finite and >= 0";
  if (!have_theta0 && beta0 != 0.0) return "a start from the prior (theta0 NULL) needs beta0 = 0";
  for (int32_t k = 0; k < T; ++k) {
    if (!ais_beta_ok(beta[k])) return "every beta must be finite and >= 0";
    if (stage_len[k] < 1) return "every stage needs a length >= 1";
    if (stage_mass && stage_mass[k] != 0 && stage_mass[k] != 1) return "stage_mass entries are 0 or 1";
    if (stage_mass && stage_mass[k] == 1 && !have_H) return "a stage that installs a mass needs H_lik";
  }
  return nullptr;
}
// Mass = beta H_lik + I / alpha, [D][D] row-major (the exact metric of a Gaussian likelihood of Hessian -H_lik tempered by beta)
inline void ais_stage_mass_matrix(double beta, const double* H_lik, int32_t D, double inv_alpha, double* mass) {
  const size_t n = (size_t)D;
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j < n; ++j) mass[i * n + j] = beta * H_lik[i * n + j] + (i == j ? inv_alpha : 0.0);  // (a product and a sum, each rounded)
}
// ... and its images, by the factorisation rmhmc_phmc_set_mass uses (mass.h): RMHMC_ERR_INVALID with *why set where that call refuses
inline int ais_stage_mass_images(double beta, const double* H_lik, int32_t D, int32_t DP, double inv_alpha, std::vector<double>& mass,
                                 std::vector<double>& Lm, std::vector<double>& Minv, const char** why) {
  mass.resize((size_t)D * (size_t)D);
  ais_stage_mass_matrix(beta, H_lik, D, inv_alpha, mass.data());
  return mass_images(mass.data(), D, DP, Lm, Minv, why);
}
