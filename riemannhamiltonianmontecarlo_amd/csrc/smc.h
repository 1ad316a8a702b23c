// smc.h — the host half of adaptive sequential Monte Carlo (include/rmhmc_smc.h): the merge and finish of conditional-ESS partials, the
// candidate grids and the bracket rule of the search, the offset U of a resampling, the blocks of the prefix sum, and the argument
// checks of the calls.  No HIP header: plain C++17, so a host compiler alone builds it (tests/helpers/smc_probe.cpp) and the library
// calls the same code.
//
// A conditional-ESS partial is double[2 + 4 J] = (a0, S0, then per j: a1, S1, a2, S2): see include/rmhmc_smc.h.
#pragma once
#include "../../include/rmhmc_smc.h"
#include "ais.h"

#include <math.h>
#include <stddef.h>
#include <stdint.h>

// ---- conditional ESS: merge and finish -----------------------------------------------------------------------------------------------
inline int64_t smc_cess_len(int32_t J) { return 2 + 4 * (int64_t)J; }
inline void smc_cess_empty(double* acc, int32_t J) {
  for (int64_t i = 0; i < smc_cess_len(J); i += 2) { acc[i] = -HUGE_VAL; acc[i + 1] = 0.0; }
}
// (a, S) <- (a, S) merged with (pa, pS).  A pair with a = -inf is the identity.
inline void smc_merge_pair(double* a, double* S, double pa, double pS) {
  if (pa == -HUGE_VAL) return;
  if (*a == -HUGE_VAL) { *a = pa; *S = pS; return; }
  const double m = *a > pa ? *a : pa;
  const double da = *a - m, dp = pa - m;  // (one of them is 0: its factor is exactly 1)
  *S = *S * exp(da) + pS * exp(dp);
  *a = m;
}
inline void smc_cess_merge(double* acc, const double* p, int32_t J) {
  for (int64_t i = 0; i < smc_cess_len(J); i += 2) smc_merge_pair(&acc[i], &acc[i + 1], p[i], p[i + 1]);
}
inline double smc_cess_frac(const double* part, int32_t j) {
  const double* q = part + 2 + 4 * (size_t)j;
  if (!(part[1] > 0.0) || !(q[1] > 0.0)) return NAN;
  const double L0 = part[0] + log(part[1]), L1 = q[0] + log(q[1]), L2 = q[2] + log(q[3]);
  return exp(2.0 * L1 - L0 - L2);
}
// merged and frac may be nullptr
inline int smc_cess_finish(const double* const* partials, int32_t k, int32_t J, double* merged, double* frac) {
  if (k < 1 || !partials || J < 1 || J > RMHMC_SMC_MAX_J) return RMHMC_ERR_INVALID;
  for (int32_t i = 0; i < k; ++i)
    if (!partials[i]) return RMHMC_ERR_INVALID;
  double acc[2 + 4 * RMHMC_SMC_MAX_J];
  smc_cess_empty(acc, J);
  for (int32_t i = 0; i < k; ++i) smc_cess_merge(acc, partials[i], J);
  if (merged) for (int64_t i = 0; i < smc_cess_len(J); ++i) merged[i] = acc[i];
  if (frac) for (int32_t j = 0; j < J; ++j) frac[j] = smc_cess_frac(acc, j);
  return RMHMC_OK;
}
inline bool smc_delta_ok(double d) { return isfinite(d) && d > 0.0; }
inline const char* smc_check_cess(int64_t n, int32_t J, const double* delta) {
  if (n < 1) return "need n >= 1";
  if (J < 1 || J > RMHMC_SMC_MAX_J || !delta) return "need 1 <= J <= 32 candidates";
  for (int32_t j = 0; j < J; ++j)
    if (!smc_delta_ok(delta[j])) return "every delta must be finite and > 0";
  return nullptr;
}

// ---- the search: RMHMC_SMC_ROUNDS rounds of RMHMC_SMC_J candidates ----------------------------------------------------------------------
struct smc_search {
  double remaining, rho;
  double lo, lo_frac;      // the largest candidate known to pass before the first that failed (0: none yet), and its frac
  double hi;               // the first candidate that failed
  double floor_delta, floor_frac;  // the smallest candidate of round 0
  int32_t round;           // the round whose grid smc_search_grid gives next
  int32_t done;
  double delta, frac;      // the result, once done
  int32_t flags;
};
inline const char* smc_check_search(int64_t n, double remaining, double rho) {
  if (n < 1) return "need n >= 1";
  if (!(remaining > 0.0) || !(remaining <= 1.0)) return "remaining must be in (0, 1]";
  if (!(rho > 0.0) || !(rho < 1.0)) return "rho must be in (0, 1)";
  return nullptr;
}
inline void smc_search_init(smc_search* s, double remaining, double rho) {
  s->remaining = remaining; s->rho = rho;
  s->lo = 0.0; s->lo_frac = NAN; s->hi = remaining;
  s->floor_delta = remaining; s->floor_frac = NAN;
  s->round = 0; s->done = 0; s->delta = NAN; s->frac = NAN; s->flags = 0;
}
inline void smc_search_grid(const smc_search* s, double delta[RMHMC_SMC_J]) {
  for (int j = 0; j < RMHMC_SMC_J; ++j) {
    if (s->round == 0) delta[j] = ldexp(s->remaining, -3 * (RMHMC_SMC_J - 1 - j));  // remaining 8^-(15 - j), exact
    else delta[j] = j == RMHMC_SMC_J - 1 ? s->hi : s->lo + (s->hi - s->lo) * ((double)(j + 1) / (double)RMHMC_SMC_J);
  }
}
// the bracket rule on the frac of the grid just evaluated
inline void smc_search_step(smc_search* s, const double delta[RMHMC_SMC_J], const double frac[RMHMC_SMC_J]) {
  int js = 0;
  while (js < RMHMC_SMC_J && frac[js] >= s->rho) ++js;  // (a NaN fails the comparison)
  if (s->round == 0) {
    s->floor_delta = delta[0]; s->floor_frac = frac[0];
    if (js == RMHMC_SMC_J) {
      s->delta = s->remaining; s->frac = frac[RMHMC_SMC_J - 1]; s->flags = RMHMC_SMC_LAST; s->done = 1;
      return;
    }
  }
  if (js == RMHMC_SMC_J) {
    s->lo = s->hi = delta[RMHMC_SMC_J - 1]; s->lo_frac = frac[RMHMC_SMC_J - 1];
  } else {
    s->hi = delta[js];
    if (js > 0) { s->lo = delta[js - 1]; s->lo_frac = frac[js - 1]; }
  }
  if (++s->round < RMHMC_SMC_ROUNDS) return;
  s->done = 1;
  if (s->lo > 0.0) { s->delta = s->lo; s->frac = s->lo_frac; }
  else { s->delta = s->floor_delta; s->frac = s->floor_frac; s->flags = RMHMC_SMC_FLOOR; }
}

// ---- resampling ----------------------------------------------------------------------------------------------------------------------------
inline uint64_t smc_splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// the offset of the resampling of stage k: the same on every shard
inline uint32_t smc_resample_u(uint64_t seed, int64_t k) {
  return (uint32_t)(smc_splitmix64(seed + 0x9E3779B97F4A7C15ull * ((uint64_t)k + 1ull)) >> 32);
}
// blocks of the prefix sum: SMC_SCAN_BLOCK entries each (256 threads of SMC_SCAN_ITEMS consecutive entries), at most SMC_SCAN_BLOCK blocks
#define SMC_SCAN_ITEMS 4
#define SMC_SCAN_BLOCK 1024
inline void smc_scan_plan(int64_t n, int64_t* nblocks, int64_t* per_block) {
  *per_block = SMC_SCAN_BLOCK;
  *nblocks = n < 1 ? 1 : (n + SMC_SCAN_BLOCK - 1) / SMC_SCAN_BLOCK;
}
// the entries [*begin, *end) of thread `thread` of block `block`
inline void smc_scan_range(int64_t n, int64_t block, int32_t thread, int64_t* begin, int64_t* end) {
  int64_t b = block * SMC_SCAN_BLOCK + (int64_t)thread * SMC_SCAN_ITEMS, e = b + SMC_SCAN_ITEMS;
  *begin = b < n ? b : n;
  *end = e < n ? e : n;
}
inline int smc_check_ancestors(int64_t n) {
  if (n < 1) return RMHMC_ERR_INVALID;
  if (n > RMHMC_SMC_MAX_N) return RMHMC_ERR_UNSUPPORTED;
  return RMHMC_OK;
}

// ---- rmhmc_smc_run: its refusals (nullptr: none) and the stages that install a mass -------------------------------------------------------
inline const char* smc_check_run(bool have_theta0, double beta0, double rho, double tau, int32_t T_max, int64_t stage_len, int64_t mass_every,
                                 bool have_H, int32_t L) {
  if (T_max < 1) return "need T_max >= 1 stages";
  if (stage_len < 1) return "need stage_len >= 1";
  if (L < 1) return "need L >= 1";
  if (!(rho > 0.0) || !(rho < 1.0)) return "rho must be in (0, 1)";
  if (!(tau >= 0.0) || !(tau <= 1.0)) return "tau must be in [0, 1]";
  if (!ais_beta_ok(beta0) || !(beta0 < 1.0)) return "beta0 must be in [0, 1)";
  if (!have_theta0 && beta0 != 0.0) return "a start from the prior (theta0 NULL) needs beta0 = 0";
  if (mass_every < 0) return "mass_every must be >= 0";
  if (mass_every > 0 && !have_H) return "a stage that installs a mass needs H_lik";
  return nullptr;
}
inline bool smc_stage_mass(int64_t k, int64_t mass_every, int32_t flags) {
  return mass_every > 0 && (k % mass_every == 0 || (flags & RMHMC_SMC_LAST) != 0);
}
