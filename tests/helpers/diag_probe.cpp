// diag_probe — csrc/diag.h on any machine: no GPU, no HIP.  Built by tests/test_diag_cpu.py with the host compiler under
// -fsanitize=address,undefined and run as a child process.
//   c++ -std=c++17 -O1 -o diag_probe tests/helpers/diag_probe.cpp
// stdin:  k H T P, then the k partials, (4 + T) * P numbers each (C99 hexadecimal floats or decimals)
// stdout: "rc <code>", then one line each of merged ((4 + T) * P), rhat, ess (P, hexadecimal floats), pairs, chains_used (P integers);
//         then "tile" lines: for every "H P" pair that follows the partials on stdin, the dimension-tile width, the LDS rows and bytes
//         and the lags per workgroup that diag.h decides.
#include "../../riemannhamiltonianmontecarlo_amd/csrc/diag.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static bool read_double(double* v) {
  char tok[128];
  if (scanf("%127s", tok) != 1) return false;
  *v = strtod(tok, nullptr);
  return true;
}

int main() {
  long long k, H, T, P;
  if (scanf("%lld %lld %lld %lld", &k, &H, &T, &P) != 4) return 2;
  const bool sane = k >= 0 && k < 1000 && T >= 0 && T < 100000 && P >= 0 && P < 100000;
  const size_t len = sane ? (size_t)(4 + T) * (size_t)P : 0;
  std::vector<std::vector<double>> parts((size_t)(sane ? k : 0), std::vector<double>(len));
  for (auto& p : parts)
    for (auto& v : p)
      if (!read_double(&v)) return 2;
  std::vector<const double*> ptrs;
  for (auto& p : parts) ptrs.push_back(p.data());
  std::vector<double> merged(len), rhat((size_t)(sane ? P : 0)), ess(rhat.size());
  std::vector<int64_t> pairs(rhat.size()), used(rhat.size());
  const int rc = diag_finish(ptrs.data(), (int32_t)k, H, T, (int32_t)P, merged.data(), rhat.data(), ess.data(), pairs.data(), used.data());
  printf("rc %d\n", rc);
  if (rc == RMHMC_OK) {
    for (double v : merged) printf("%a ", v);
    printf("\n");
    for (double v : rhat) printf("%a ", v);
    printf("\n");
    for (double v : ess) printf("%a ", v);
    printf("\n");
    for (int64_t v : pairs) printf("%lld ", (long long)v);
    printf("\n");
    for (int64_t v : used) printf("%lld ", (long long)v);
    printf("\n");
    // the NULL outputs are optional: the same call with none of them
    if (diag_finish(ptrs.data(), (int32_t)k, H, T, (int32_t)P, nullptr, nullptr, nullptr, nullptr, nullptr) != RMHMC_OK) return 3;
  }
  long long h, p;
  while (scanf("%lld %lld", &h, &p) == 2) {
    const int tw = diag_tile_width(h, (int32_t)p);
    printf("tile %lld %lld %d %lld %lld %lld\n", h, p, tw, (long long)diag_lds_rows(h), tw ? (long long)diag_lds_bytes(h, tw) : 0,
           tw ? (long long)diag_lags_per_block(tw) : 0);
  }
  return 0;
}
