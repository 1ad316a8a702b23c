// mass.h — the shared mass matrix of the fixed-metric HMC sampler (include/rmhmc_phmc.h) on the host: the check of the caller's
// matrix, its lower Cholesky factor Lm (Mass = Lm Lm') and the inverse Mass^-1, as the two zero-padded [DP][DP] row-major images
// rmhmc_phmc_set_mass uploads (phmc.hip.h multiplies a batch of chains with them on the matrix cores).
// No HIP header: plain C++17 for the host compiler, so the factorisation can be tested on a machine without a GPU
// (tests/helpers/mass_probe.cpp).
#pragma once
#include "../../include/rmhmc.h"

#include <cmath>
#include <cstddef>
#include <vector>

// mass: [D][D] row-major, of which the lower triangle is read, or nullptr: the identity.  Lm and Minv come back [DP][DP] with zero
// padding (Minv exactly symmetric).  RMHMC_ERR_INVALID with *why set, and both images untouched, for a non-finite entry or a pivot <= 0.
inline int mass_images(const double* mass, int D, int DP, std::vector<double>& Lm, std::vector<double>& Minv, const char** why) {
  const size_t n = (size_t)D, ld = (size_t)DP;
  if (D < 1 || DP < D) { *why = "mass: bad shape"; return RMHMC_ERR_INVALID; }
  std::vector<double> L(ld * ld, 0.0), Li(n * n, 0.0), Mi(ld * ld, 0.0);
  if (!mass) {  // exact zeros and ones: the products with these images are exact
    for (size_t i = 0; i < n; ++i) L[i * ld + i] = Mi[i * ld + i] = 1.0;
    Lm.swap(L); Minv.swap(Mi);
    return RMHMC_OK;
  }
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j <= i; ++j)
      if (!std::isfinite(mass[i * n + j])) { *why = "mass: non-finite entry"; return RMHMC_ERR_INVALID; }
  for (size_t j = 0; j < n; ++j) {  // Cholesky-Crout, column by column
    double d = mass[j * n + j];
    for (size_t k = 0; k < j; ++k) d -= L[j * ld + k] * L[j * ld + k];
    if (!(d > 0.0) || !std::isfinite(d)) { *why = "mass: not positive definite (pivot <= 0)"; return RMHMC_ERR_INVALID; }
    const double piv = std::sqrt(d);
    L[j * ld + j] = piv;
    for (size_t i = j + 1; i < n; ++i) {
      double s = mass[i * n + j];
      for (size_t k = 0; k < j; ++k) s -= L[i * ld + k] * L[j * ld + k];
      L[i * ld + j] = s / piv;
    }
  }
  for (size_t j = 0; j < n; ++j) {  // Li = Lm^-1 (lower), by forward substitution on the columns of the identity
    Li[j * n + j] = 1.0 / L[j * ld + j];
    for (size_t i = j + 1; i < n; ++i) {
      double s = 0.0;
      for (size_t k = j; k < i; ++k) s -= L[i * ld + k] * Li[k * n + j];
      Li[i * n + j] = s / L[i * ld + i];
    }
  }
  for (size_t i = 0; i < n; ++i)  // Mass^-1 = Li' Li
    for (size_t j = 0; j <= i; ++j) {
      double s = 0.0;
      for (size_t k = i; k < n; ++k) s += Li[k * n + i] * Li[k * n + j];
      if (!std::isfinite(s)) { *why = "mass: the inverse overflows"; return RMHMC_ERR_INVALID; }
      Mi[i * ld + j] = Mi[j * ld + i] = s;
    }
  Lm.swap(L); Minv.swap(Mi);
  return RMHMC_OK;
}
