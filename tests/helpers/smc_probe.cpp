// smc_probe — csrc/smc.h on any machine: no GPU, no HIP.  Built by tests/test_smc_cpu.py with the host compiler under
// -fsanitize=address,undefined and run as a child process.
//   c++ -std=c++17 -O1 -o smc_probe tests/helpers/smc_probe.cpp
// stdin: commands, one after another (numbers as C99 hexadecimal floats or decimals); stdout: one answer per command.
//   grid round remaining lo hi                 -> "grid" and the 16 candidates of that round
//   search remaining rho  <16 frac per round>  -> per round "round <16 candidates>", then "result delta frac flags"; reads a round's frac only
//                                                 when the search asks for that round
//   u seed k                                   -> "u U"
//   cess k J  <k partials of 2 + 4 J numbers>  -> "cess rc" then, for rc 0, merged (2 + 4 J) and frac (J), one line each
//   plan n                                     -> "plan nblocks per_block"
//   range n block thread                       -> "range begin end"
//   cover n                                    -> "cover ok" if the ranges of every thread of every block, in order, are 0 .. n without a gap
//   checkrun have_theta0 beta0 rho tau T_max stage_len mass_every have_H L   -> "check ok" or "check <reason>"
//   checkcess n J <J deltas> | checksearch n remaining rho                   -> the same
//   checkanc n                                 -> "checkanc rc"
//   smass k mass_every flags                   -> "smass 0|1"
#include "../../riemannhamiltonianmontecarlo_amd/csrc/smc.h"

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

static void print_row(const double* v, size_t n) {
  for (size_t i = 0; i < n; ++i) printf("%a ", v[i]);
  printf("\n");
}

int main() {
  char cmd[32];
  int seen = 0;
  while (scanf("%31s", cmd) == 1) {
    ++seen;
    if (!strcmp(cmd, "grid")) {
      long long rnd;
      smc_search s;
      double remaining, lo, hi;
      if (scanf("%lld", &rnd) != 1 || !read_double(&remaining) || !read_double(&lo) || !read_double(&hi)) return 2;
      smc_search_init(&s, remaining, 0.5);
      s.round = (int32_t)rnd; s.lo = lo; s.hi = hi;
      double d[RMHMC_SMC_J];
      smc_search_grid(&s, d);
      printf("grid ");
      print_row(d, RMHMC_SMC_J);
    } else if (!strcmp(cmd, "search")) {
      double remaining, rho;
      if (!read_double(&remaining) || !read_double(&rho)) return 2;
      smc_search s;
      smc_search_init(&s, remaining, rho);
      int rounds = 0;
      while (!s.done) {
        if (++rounds > RMHMC_SMC_ROUNDS) return 6;  // the search ends within its rounds
        double d[RMHMC_SMC_J], f[RMHMC_SMC_J];
        smc_search_grid(&s, d);
        for (double& v : f)
          if (!read_double(&v)) return 2;
        printf("round ");
        print_row(d, RMHMC_SMC_J);
        smc_search_step(&s, d, f);
      }
      printf("result %a %a %d\n", s.delta, s.frac, (int)s.flags);
    } else if (!strcmp(cmd, "u")) {
      unsigned long long seed;
      long long k;
      if (scanf("%llu %lld", &seed, &k) != 2) return 2;
      printf("u %llu\n", (unsigned long long)smc_resample_u((uint64_t)seed, (int64_t)k));
    } else if (!strcmp(cmd, "cess")) {
      long long k, J;
      if (scanf("%lld %lld", &k, &J) != 2) return 2;
      const bool sane = k >= 0 && k < 1000 && J >= 1 && J <= RMHMC_SMC_MAX_J;
      const size_t len = sane ? (size_t)smc_cess_len((int32_t)J) : 0;
      std::vector<std::vector<double>> parts((size_t)(sane ? k : 0), std::vector<double>(len));
      for (auto& q : parts)
        for (auto& v : q)
          if (!read_double(&v)) return 2;
      std::vector<const double*> ptrs;
      for (auto& q : parts) ptrs.push_back(q.data());
      std::vector<double> merged(len ? len : 1, -7.0), frac(sane ? (size_t)J : 1, -7.0);
      const int rc = smc_cess_finish(ptrs.data(), (int32_t)k, (int32_t)J, merged.data(), frac.data());
      printf("cess %d\n", rc);
      if (rc == RMHMC_OK) {
        print_row(merged.data(), len);
        print_row(frac.data(), (size_t)J);
        if (smc_cess_finish(ptrs.data(), (int32_t)k, (int32_t)J, nullptr, nullptr) != RMHMC_OK) return 3;  // the outputs are optional
      } else if (merged[0] != -7.0 || frac[0] != -7.0) {
        return 4;  // a refusal writes nothing
      }
    } else if (!strcmp(cmd, "plan")) {
      long long n;
      if (scanf("%lld", &n) != 1 || n < 1) return 2;
      int64_t nb, pb;
      smc_scan_plan(n, &nb, &pb);
      printf("plan %lld %lld\n", (long long)nb, (long long)pb);
    } else if (!strcmp(cmd, "range")) {
      long long n, block, thread;
      if (scanf("%lld %lld %lld", &n, &block, &thread) != 3) return 2;
      int64_t b, e;
      smc_scan_range(n, block, (int32_t)thread, &b, &e);
      printf("range %lld %lld\n", (long long)b, (long long)e);
    } else if (!strcmp(cmd, "cover")) {
      long long n;
      if (scanf("%lld", &n) != 1 || n < 1) return 2;
      int64_t nb, pb, at = 0;
      smc_scan_plan(n, &nb, &pb);
      bool ok = pb == SMC_SCAN_BLOCK && (n > RMHMC_SMC_MAX_N || nb <= SMC_SCAN_BLOCK);  // (the block totals are scanned by one block)
      for (int64_t blk = 0; blk < nb && ok; ++blk)
        for (int32_t t = 0; t < 256 && ok; ++t) {
          int64_t b, e;
          smc_scan_range(n, blk, t, &b, &e);
          ok = b == at && e >= b && e - b <= SMC_SCAN_ITEMS;
          at = e;
        }
      printf("cover %s\n", ok && at == n ? "ok" : "bad");
    } else if (!strcmp(cmd, "checkrun")) {
      long long have_theta0, T_max, stage_len, mass_every, have_H, L;
      double beta0, rho, tau;
      if (scanf("%lld", &have_theta0) != 1 || !read_double(&beta0) || !read_double(&rho) || !read_double(&tau) ||
          scanf("%lld %lld %lld %lld %lld", &T_max, &stage_len, &mass_every, &have_H, &L) != 5)
        return 2;
      const char* why = smc_check_run(have_theta0 != 0, beta0, rho, tau, (int32_t)T_max, stage_len, mass_every, have_H != 0, (int32_t)L);
      printf("check %s\n", why ? why : "ok");
    } else if (!strcmp(cmd, "checkcess")) {
      long long n, J;
      if (scanf("%lld %lld", &n, &J) != 2 || J > 1000) return 2;
      std::vector<double> d((size_t)(J > 0 ? J : 0));
      for (auto& v : d)
        if (!read_double(&v)) return 2;
      const char* why = smc_check_cess(n, (int32_t)J, d.data());
      printf("check %s\n", why ? why : "ok");
    } else if (!strcmp(cmd, "checksearch")) {
      long long n;
      double remaining, rho;
      if (scanf("%lld", &n) != 1 || !read_double(&remaining) || !read_double(&rho)) return 2;
      const char* why = smc_check_search(n, remaining, rho);
      printf("check %s\n", why ? why : "ok");
    } else if (!strcmp(cmd, "checkanc")) {
      long long n;
      if (scanf("%lld", &n) != 1) return 2;
      printf("checkanc %d\n", smc_check_ancestors(n));
    } else if (!strcmp(cmd, "smass")) {
      long long k, every, flags;
      if (scanf("%lld %lld %lld", &k, &every, &flags) != 3) return 2;
      printf("smass %d\n", smc_stage_mass(k, every, (int32_t)flags) ? 1 : 0);
    } else {
      return 2;
    }
  }
  return seen ? 0 : 2;
}
