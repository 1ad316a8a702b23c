// Stand-alone driver of csrc/quant.h for tests/test_quant_cpu.py: built with the host compiler under AddressSanitizer and UBSan and run
// as a child process.  Commands on stdin (doubles as C hex floats, keys and prefixes as hex integers), one answer block each:
//   keys n  x[n]                                       -> "key <key> <unkey(key)> <finite> <digit r = 0..7>" per value
//   plan P Q  m[P] probs[Q]                            -> "rc <rc>", then rank [2Q][P] and frac [Q][P], a row per line
//   step P K round parts  prefix[K P] rank[K P] hists  -> "rc <rc>", then prefix and rank as left by the call
//   finish P Q  prefix[2Q P] frac[Q P] m[P]            -> "rc <rc>", then quant [Q][P]
//   select N P Q parts  probs[Q] bounds[parts + 1] x[N P] -> the whole eight-round loop; the histograms of every part (rows bounds[i] ..
//        bounds[i + 1]) are filled here by a plain loop with quant_key, quant_match and quant_digit; "rc <rc>", m [P], the order
//        statistics [2Q][P] and quant [Q][P]
// No input: exit status 2.
#include "../../riemannhamiltonianmontecarlo_amd/csrc/quant.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

static bool rd(double* v) { return scanf("%la", v) == 1; }
static bool rd(int64_t* v) { return scanf("%" SCNd64, v) == 1; }
static bool rd(uint64_t* v) { return scanf("%" SCNx64, v) == 1; }
template <typename T>
static bool rdv(std::vector<T>& v) {
  for (T& e : v)
    if (!rd(&e)) return false;
  return true;
}
static void row(const double* v, size_t n) {
  for (size_t i = 0; i < n; ++i) printf("%a ", v[i]);
  printf("\n");
}
static void row(const int64_t* v, size_t n) {
  for (size_t i = 0; i < n; ++i) printf("%" PRId64 " ", v[i]);
  printf("\n");
}
static void row(const uint64_t* v, size_t n) {
  for (size_t i = 0; i < n; ++i) printf("%" PRIx64 " ", v[i]);
  printf("\n");
}

// the histogram partial of rows a .. b of x [N][P]: what k_quant_hist counts, as a plain loop
static void fill(const std::vector<double>& x, int64_t a, int64_t b, int P, int round, const std::vector<uint64_t>& prefix, int K,
                 std::vector<double>& h) {
  const int Kh = round ? K : 1;
  h.assign((size_t)Kh * P * QUANT_BINS, 0.0);
  for (int64_t r = a; r < b; ++r)
    for (int d = 0; d < P; ++d) {
      const uint64_t key = quant_key(x[(size_t)r * P + d]);
      if (!quant_key_finite(key)) continue;
      for (int k = 0; k < Kh; ++k)
        if (quant_match(key, round ? prefix[(size_t)k * P + d] : 0, round)) h[((size_t)k * P + d) * QUANT_BINS + quant_digit(key, round)] += 1.0;
    }
}

int main() {
  char cmd[16];
  int seen = 0;
  while (scanf("%15s", cmd) == 1) {
    ++seen;
    if (!strcmp(cmd, "keys")) {
      int64_t n;
      if (!rd(&n)) return 3;
      for (int64_t i = 0; i < n; ++i) {
        double x;
        if (!rd(&x)) return 3;
        const uint64_t k = quant_key(x);
        printf("key %" PRIx64 " %a %d", k, quant_unkey(k), (int)quant_key_finite(k));
        for (int r = 0; r < 8; ++r) printf(" %d", quant_digit(k, r));
        printf("\n");
      }
    } else if (!strcmp(cmd, "plan")) {
      int64_t P, Q;
      if (!rd(&P) || !rd(&Q) || P < 0 || Q < 0 || P > 4096 || Q > 64) return 3;
      std::vector<int64_t> m((size_t)P), rank((size_t)(2 * Q * P), -7);
      std::vector<double> probs((size_t)Q), frac((size_t)(Q * P), -7.0);
      if (!rdv(m) || !rdv(probs)) return 3;
      printf("rc %d\n", quant_plan(m.data(), probs.data(), (int32_t)Q, (int32_t)P, rank.data(), frac.data()));
      for (int64_t j = 0; j < 2 * Q; ++j) row(rank.data() + j * P, (size_t)P);
      for (int64_t j = 0; j < Q; ++j) row(frac.data() + j * P, (size_t)P);
    } else if (!strcmp(cmd, "step")) {
      int64_t P, K, round, parts;
      if (!rd(&P) || !rd(&K) || !rd(&round) || !rd(&parts) || P < 1 || K < 1 || parts < 0 || P > 4096 || K > 64 || parts > 64) return 3;
      std::vector<uint64_t> prefix((size_t)(K * P));
      std::vector<int64_t> rank((size_t)(K * P));
      if (!rdv(prefix) || !rdv(rank)) return 3;
      const size_t len = (size_t)((round > 0 ? K : 1) * P) * QUANT_BINS;
      std::vector<std::vector<double>> h((size_t)parts, std::vector<double>(len));
      std::vector<const double*> ptr;
      for (auto& v : h) {
        if (!rdv(v)) return 3;
        ptr.push_back(v.data());
      }
      printf("rc %d\n", quant_step(ptr.data(), (int32_t)parts, (int32_t)P, (int32_t)K, (int32_t)round, prefix.data(), rank.data()));
      row(prefix.data(), prefix.size());
      row(rank.data(), rank.size());
    } else if (!strcmp(cmd, "finish")) {
      int64_t P, Q;
      if (!rd(&P) || !rd(&Q) || P < 1 || Q < 1 || P > 4096 || Q > 64) return 3;
      std::vector<uint64_t> prefix((size_t)(2 * Q * P));
      std::vector<double> frac((size_t)(Q * P)), quant((size_t)(Q * P), -7.0);
      std::vector<int64_t> m((size_t)P);
      if (!rdv(prefix) || !rdv(frac) || !rdv(m)) return 3;
      printf("rc %d\n", quant_finish(prefix.data(), frac.data(), m.data(), (int32_t)Q, (int32_t)P, quant.data()));
      for (int64_t j = 0; j < Q; ++j) row(quant.data() + j * P, (size_t)P);
    } else if (!strcmp(cmd, "select")) {
      int64_t N, P, Q, parts;
      if (!rd(&N) || !rd(&P) || !rd(&Q) || !rd(&parts) || N < 0 || P < 1 || Q < 1 || Q > 8 || parts < 1 || parts > 64 || P > 4096) return 3;
      std::vector<double> probs((size_t)Q), x((size_t)(N * P));
      std::vector<int64_t> bounds((size_t)parts + 1);
      if (!rdv(probs) || !rdv(bounds) || !rdv(x)) return 3;
      for (int64_t i = 0; i < parts; ++i)
        if (bounds[(size_t)i] < 0 || bounds[(size_t)i] > bounds[(size_t)i + 1] || bounds[(size_t)i + 1] > N) return 3;
      const int K = (int)(2 * Q);
      std::vector<uint64_t> prefix((size_t)(K * P), 0);
      std::vector<int64_t> rank((size_t)(K * P)), m((size_t)P);
      std::vector<double> frac((size_t)(Q * P)), quant((size_t)(Q * P)), order((size_t)(K * P));
      std::vector<std::vector<double>> h((size_t)parts);
      int rc = RMHMC_OK;
      for (int round = 0; round < 8 && rc == RMHMC_OK; ++round) {
        std::vector<const double*> ptr;
        for (int64_t i = 0; i < parts; ++i) {
          fill(x, bounds[(size_t)i], bounds[(size_t)i + 1], (int)P, round, prefix, K, h[(size_t)i]);
          ptr.push_back(h[(size_t)i].data());
        }
        if (round == 0) {
          std::vector<double> sum(h[0].size(), 0.0);
          for (auto& v : h)
            for (size_t i = 0; i < v.size(); ++i) sum[i] += v[i];
          quant_totals(sum.data(), (int32_t)P, m.data());
          rc = quant_plan(m.data(), probs.data(), (int32_t)Q, (int32_t)P, rank.data(), frac.data());
        }
        if (rc == RMHMC_OK) rc = quant_step(ptr.data(), (int32_t)parts, (int32_t)P, K, round, prefix.data(), rank.data());
      }
      if (rc == RMHMC_OK) rc = quant_finish(prefix.data(), frac.data(), m.data(), (int32_t)Q, (int32_t)P, quant.data());
      printf("rc %d\n", rc);
      for (size_t i = 0; i < order.size(); ++i) order[i] = m[i % (size_t)P] > 0 ? quant_unkey(prefix[i]) : NAN;
      row(m.data(), m.size());
      for (int j = 0; j < K; ++j) row(order.data() + (size_t)j * P, (size_t)P);
      for (int64_t j = 0; j < Q; ++j) row(quant.data() + j * P, (size_t)P);
    } else {
      return 3;
    }
  }
  return seen ? 0 : 2;
}
