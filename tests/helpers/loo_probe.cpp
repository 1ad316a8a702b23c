// loo_probe — csrc/loo.h on any machine: no GPU, no HIP.  Built by tests/test_loo_cpu.py with the host compiler under
// -fsanitize=address,undefined and run as a child process.
//   c++ -std=c++17 -O1 -o loo_probe tests/helpers/loo_probe.cpp
// stdin: commands, one after another (numbers as C99 hexadecimal floats or decimals); stdout: one answer per command.
//   plan C <m, C integers>                   -> "plan rc" then, for rc 0, tail_len and rank, one line each (sentinels untouched otherwise)
//   finish k C have_fit <k partials of 5 C numbers> <fit, 4 C numbers, and body, 2 C numbers, when have_fit>
//                                            -> "finish rc k_mid k_high" then merged (5 C), elpd_loo, p_loo, pareto_k, lppd, p_waic,
//                                               elpd_waic (C each), totals (6) and draws_used (C), one line each
//   refusals                                 -> "refusals" and the codes of every refusal of loo_plan and loo_finish
//   consts                                   -> "consts LOO_MAX_COLS LOO_MAX_TAIL LOO_MAX_D LOO_BLOCK_ROWS LOO_MAX_BLOCKS LOO_ROW_LANES LOO_DRAWS"
//   kplan N D                                -> "kplan lblocks vblocks draws_per_vblock rblocks rows_per_block ksteps cols_per_block"
//   check C D <x, C D numbers> <t, C numbers> -> "check ok" or "check <reason>"
#include "../../riemannhamiltonianmontecarlo_amd/csrc/loo.h"

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

static void print_ints(const std::vector<int64_t>& v) {
  for (int64_t x : v) printf("%lld ", (long long)x);
  printf("\n");
}

int main() {
  char cmd[32];
  int seen = 0;
  while (scanf("%31s", cmd) == 1) {
    ++seen;
    if (!strcmp(cmd, "plan")) {
      long long C;
      if (scanf("%lld", &C) != 1 || C < 1 || C > 1000) return 2;
      std::vector<int64_t> m((size_t)C), tl((size_t)C, -7), rank((size_t)C, -7);
      for (auto& v : m) {
        long long x;
        if (scanf("%lld", &x) != 1) return 2;
        v = x;
      }
      const int rc = loo_plan(m.data(), (int32_t)C, tl.data(), rank.data());
      printf("plan %d\n", rc);
      if (rc == RMHMC_OK) {
        print_ints(tl);
        print_ints(rank);
      } else {
        for (size_t i = 0; i < (size_t)C; ++i)
          if (tl[i] != -7 || rank[i] != -7) return 4;  // a refusal writes nothing
      }
    } else if (!strcmp(cmd, "finish")) {
      long long k, C, have_fit;
      if (scanf("%lld %lld %lld", &k, &C, &have_fit) != 3 || k < 1 || k > 100 || C < 1 || C > 100000) return 2;
      std::vector<std::vector<double>> parts((size_t)k, std::vector<double>((size_t)(5 * C)));
      for (auto& q : parts)
        for (auto& v : q)
          if (!read_double(&v)) return 2;
      std::vector<double> fit((size_t)(4 * C)), body((size_t)(2 * C));
      if (have_fit) {
        for (auto& v : fit)
          if (!read_double(&v)) return 2;
        for (auto& v : body)
          if (!read_double(&v)) return 2;
      }
      std::vector<const double*> ptrs;
      for (auto& q : parts) ptrs.push_back(q.data());
      const size_t n = (size_t)C;
      std::vector<double> merged(5 * n, -7.0), el(n, -7.0), pl(n, -7.0), kh(n, -7.0), lp(n, -7.0), pw(n, -7.0), ew(n, -7.0), totals(6, -7.0);
      std::vector<int64_t> kc(2, -7), used(n, -7);
      const double* f = have_fit ? fit.data() : nullptr;
      const double* b = have_fit ? body.data() : nullptr;
      const int rc = loo_finish(ptrs.data(), (int32_t)k, C, f, b, merged.data(), el.data(), pl.data(), kh.data(), lp.data(), pw.data(), ew.data(),
                                totals.data(), kc.data(), used.data());
      printf("finish %d %lld %lld\n", rc, (long long)kc[0], (long long)kc[1]);
      if (rc != RMHMC_OK) return 3;
      print_row(merged);
      print_row(el);
      print_row(pl);
      print_row(kh);
      print_row(lp);
      print_row(pw);
      print_row(ew);
      print_row(totals);
      print_ints(used);
      // the outputs are optional: the same call with none of them
      if (loo_finish(ptrs.data(), (int32_t)k, C, f, b, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) !=
          RMHMC_OK)
        return 3;
    } else if (!strcmp(cmd, "refusals")) {
      double part[5] = {3.0, -0.5, 0.25, 1.5, -1.0};
      const double fit[4] = {0.3, 1.0, 2.0, 1.0}, body[2] = {1.0, 0.5};
      const double* good[2] = {part, part};
      const double* holed[2] = {part, nullptr};
      double out[9] = {-7.0, -7.0, -7.0, -7.0, -7.0, -7.0, -7.0, -7.0, -7.0}, merged[5] = {-7.0, -7.0, -7.0, -7.0, -7.0}, totals[6] = {-7.0, -7.0, -7.0, -7.0, -7.0, -7.0};
      int64_t kc[2] = {-7, -7}, used = -7;
      auto fin = [&](const double* const* p, int32_t k, int64_t C, const double* f, const double* b) {
        return loo_finish(p, k, C, f, b, merged, &out[0], &out[1], &out[2], &out[3], &out[4], &out[5], totals, kc, &used);
      };
      const int r0 = fin(good, 0, 1, fit, body), r1 = fin(good, 2, 0, fit, body), r2 = fin(holed, 2, 1, fit, body), r3 = fin(nullptr, 2, 1, fit, body);
      const int r4 = fin(good, 2, 1, fit, nullptr), r5 = fin(good, 2, 1, nullptr, body);
      for (double v : out)
        if (v != -7.0) return 4;
      for (double v : merged)
        if (v != -7.0) return 4;
      for (double v : totals)
        if (v != -7.0) return 4;
      if (kc[0] != -7 || kc[1] != -7 || used != -7) return 4;
      int64_t m[2] = {100, 200}, neg[2] = {100, -1}, big[2] = {100, 29826162}, tl[2] = {-7, -7}, rank[2] = {-7, -7};
      const int p0 = loo_plan(nullptr, 2, tl, rank), p1 = loo_plan(m, 2, nullptr, rank), p2 = loo_plan(m, 2, tl, nullptr), p3 = loo_plan(m, 0, tl, rank);
      const int p4 = loo_plan(neg, 2, tl, rank), p5 = loo_plan(big, 2, tl, rank);
      if (tl[0] != -7 || tl[1] != -7 || rank[0] != -7 || rank[1] != -7) return 4;
      printf("refusals %d %d %d %d %d %d %d %d %d %d %d %d\n", r0, r1, r2, r3, r4, r5, p0, p1, p2, p3, p4, p5);
    } else if (!strcmp(cmd, "consts")) {
      printf("consts %d %d %d %d %d %d %d\n", LOO_MAX_COLS, LOO_MAX_TAIL, LOO_MAX_D, LOO_BLOCK_ROWS, LOO_MAX_BLOCKS, LOO_ROW_LANES, LOO_DRAWS);
    } else if (!strcmp(cmd, "kplan")) {
      long long N, D;
      if (scanf("%lld %lld", &N, &D) != 2 || N < 1 || D < 1 || D > LOO_MAX_D) return 2;
      const loo_plan_t p = loo_kernel_plan(N, (int32_t)D);
      printf("kplan %lld %lld %lld %lld %lld %d %d\n", (long long)p.lblocks, (long long)p.vblocks, (long long)p.draws_per_vblock, (long long)p.rblocks,
             (long long)p.rows_per_block, (int)p.ksteps, (int)loo_cols_per_block(N));
    } else if (!strcmp(cmd, "check")) {
      long long C, D;
      if (scanf("%lld %lld", &C, &D) != 2 || C < 1 || C > 10000 || D < 1 || D > LOO_MAX_D) return 2;
      std::vector<double> x((size_t)(C * D)), t((size_t)C);
      for (auto& v : x)
        if (!read_double(&v)) return 2;
      for (auto& v : t)
        if (!read_double(&v)) return 2;
      const char* why = loo_check_rows(x.data(), t.data(), C, (int32_t)D);
      printf("check %s\n", why ? why : "ok");
    } else {
      return 2;
    }
  }
  return seen ? 0 : 2;
}
