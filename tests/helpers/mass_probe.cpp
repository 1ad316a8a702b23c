// mass_probe — csrc/mass.h on any machine: no GPU, no HIP.  Built by tests/test_phmc_cpu.py with the host compiler under
// -fsanitize=address,undefined and run as a child process.
//   c++ -std=c++17 -O1 -o mass_probe tests/helpers/mass_probe.cpp
// stdin:  D DP, then "identity" or the D * D entries of the matrix, row-major (C99 hexadecimal floats, decimals, nan, inf)
// stdout: "rc <code> <message>", then for RMHMC_OK one line each of Lm and Mass^-1 ([DP][DP], hexadecimal floats)
#include "../../riemannhamiltonianmontecarlo_amd/csrc/mass.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

int main() {
  int D, DP;
  if (scanf("%d %d", &D, &DP) != 2 || D < 1 || D > 4096 || DP < D || DP > 4096) return 2;
  std::vector<double> m((size_t)D * D);
  bool identity = false;
  for (size_t i = 0; i < m.size(); ++i) {
    char tok[128];
    if (scanf("%127s", tok) != 1) return 2;
    if (i == 0 && !strcmp(tok, "identity")) { identity = true; break; }
    m[i] = strtod(tok, nullptr);
  }
  // the images start out with a marker: a refusal must leave them as they are
  std::vector<double> Lm(3, 7.0), Mi(3, 7.0);
  const char* why = "";
  const int rc = mass_images(identity ? nullptr : m.data(), D, DP, Lm, Mi, &why);
  printf("rc %d %s\n", rc, why);
  if (rc != RMHMC_OK) return (Lm.size() == 3 && Mi.size() == 3 && Lm[0] == 7.0 && Mi[2] == 7.0) ? 0 : 3;
  if (Lm.size() != (size_t)DP * DP || Mi.size() != (size_t)DP * DP) return 3;
  for (double v : Lm) printf("%a ", v);
  printf("\n");
  for (double v : Mi) printf("%a ", v);
  printf("\n");
  return 0;
}
