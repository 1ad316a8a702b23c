// adapt_probe — csrc/adapt.h on any machine: no GPU, no HIP.  Built by tests/test_adapt_cpu.py with the host compiler under
// -fsanitize=address,undefined and run as a child process.
//   c++ -std=c++17 -O1 -o adapt_probe tests/helpers/adapt_probe.cpp
// stdin: commands, one after another (numbers as C99 hexadecimal floats or decimals); stdout: one answer per command.
//   finish k P  <k partials of (2 + P) * P numbers>   -> "finish rc m" then merged ((2 + P) * P), mean (P), cov (P * P), one line each
//   mass P m  <cov, P * P numbers>                    -> "mass rc" then, for rc 0, the mass (P * P) on one line
//   da eps0 delta gamma t0 kappa count  <count tokens: an acceptance statistic, or "restart">
//                                                       -> per token "da rc eps_next eps_bar t Hbar logepsbar mu" (a restart: at eps_next, factor 1)
//   sched warmup window                                -> "sched W kind_0 .. kind_{W-1}" (W = 0: refused)
//   plan N P                                           -> "plan nblocks rows_per_block nblocks_sums rows_per_block_sums"
#include "../../riemannhamiltonianmontecarlo_amd/csrc/adapt.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static bool read_double(double* v) {
  char tok[128];
  if (scanf("%127s", tok) != 1) return false;
  *v = strtod(tok, nullptr);
  return true;
}

static void print_row(const std::vector<double>& v) {
  for (double x : v) printf("%a ", x);
  printf("\n");
}

int main() {
  char cmd[32];
  int seen = 0;
  while (scanf("%31s", cmd) == 1) {
    ++seen;
    if (!strcmp(cmd, "finish")) {
      long long k, P;
      if (scanf("%lld %lld", &k, &P) != 2) return 2;
      const bool sane = k >= 0 && k < 1000 && P >= 0 && P < 2000;
      const size_t p = sane ? (size_t)P : 0, len = (2 + p) * p;
      std::vector<std::vector<double>> parts((size_t)(sane ? k : 0), std::vector<double>(len));
      for (auto& q : parts)
        for (auto& v : q)
          if (!read_double(&v)) return 2;
      std::vector<const double*> ptrs;
      for (auto& q : parts) ptrs.push_back(q.data());
      std::vector<double> merged(len), mean(p), cov(p * p);
      int64_t m = -1;
      const int rc = cov_finish(ptrs.data(), (int32_t)k, (int32_t)P, merged.data(), mean.data(), cov.data(), &m);
      printf("finish %d %lld\n", rc, (long long)m);
      if (rc == RMHMC_OK) {
        print_row(merged);
        print_row(mean);
        print_row(cov);
        // the outputs are optional: the same call with none of them
        if (cov_finish(ptrs.data(), (int32_t)k, (int32_t)P, nullptr, nullptr, nullptr, nullptr) != RMHMC_OK) return 3;
      }
    } else if (!strcmp(cmd, "mass")) {
      long long P, m;
      if (scanf("%lld %lld", &P, &m) != 2 || P < 1 || P > 2000) return 2;
      std::vector<double> cov((size_t)(P * P)), mass((size_t)(P * P), -7.0);
      for (auto& v : cov)
        if (!read_double(&v)) return 2;
      const char* why = nullptr;
      const int rc = adapt_mass(cov.data(), m, (int32_t)P, mass.data(), &why);
      printf("mass %d\n", rc);
      if (rc == RMHMC_OK) {
        print_row(mass);
      } else {
        for (double v : mass)
          if (v != -7.0) return 4;  // a refusal leaves the caller's matrix alone
        if (!why || !*why) return 5;
      }
    } else if (!strcmp(cmd, "da")) {
      double eps0, delta, gamma, t0, kappa;
      long long count;
      if (!read_double(&eps0) || !read_double(&delta) || !read_double(&gamma) || !read_double(&t0) || !read_double(&kappa)) return 2;
      if (scanf("%lld", &count) != 1) return 2;
      double state[4] = {-1.0, -1.0, -1.0, -1.0};
      int rc = adapt_init(state, eps0, ADAPT_FACTOR_START);
      double eps = eps0, bar = eps0;
      for (long long i = 0; i < count; ++i) {
        char tok[128];
        if (scanf("%127s", tok) != 1) return 2;
        if (rc == RMHMC_OK) {
          if (!strcmp(tok, "restart")) rc = adapt_init(state, eps, ADAPT_FACTOR_RESTART);
          else rc = adapt_step(state, strtod(tok, nullptr), delta, gamma, t0, kappa, &eps, &bar);
        }
        printf("da %d %a %a %a %a %a %a\n", rc, eps, bar, state[0], state[1], state[2], state[3]);
        if (rc != RMHMC_OK) rc = RMHMC_OK;  // a refusal leaves the state alone: the sequence goes on from it
      }
    } else if (!strcmp(cmd, "sched")) {
      long long warmup, window;
      if (scanf("%lld %lld", &warmup, &window) != 2) return 2;
      const int64_t W = adapt_schedule(warmup, window, nullptr, nullptr);
      std::vector<int64_t> len((size_t)W);
      std::vector<int32_t> kind((size_t)W);
      if (adapt_schedule(warmup, window, len.data(), kind.data()) != W) return 6;
      printf("sched %lld", (long long)W);
      for (int64_t w = 0; w < W; ++w) {
        if (len[(size_t)w] != window) return 6;
        printf(" %d", (int)kind[(size_t)w]);
      }
      printf("\n");
    } else if (!strcmp(cmd, "plan")) {
      long long N, P;
      if (scanf("%lld %lld", &N, &P) != 2 || N < 1 || P < 1) return 2;
      int64_t nb, rpb, nb1, rpb1;
      cov_plan(N, (int32_t)P, &nb, &rpb);
      cov_plan_sums(N, &nb1, &rpb1);
      printf("plan %lld %lld %lld %lld\n", (long long)nb, (long long)rpb, (long long)nb1, (long long)rpb1);
    } else {
      return 2;
    }
  }
  return seen ? 0 : 2;
}
