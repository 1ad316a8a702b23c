// quant.h — the host half of the posterior quantiles (include/rmhmc_quant.h): the key and its inverse, the digit of a round, the plan
// of the targets, one round of the select on merged histograms, the finish, and the shape constants of the kernel of quant.hip.h.
// No HIP header: plain C++17, so a host compiler alone builds it (tests/helpers/quant_probe.cpp) and the library calls the same code
// (rmhmc_quant_plan, rmhmc_quant_step, rmhmc_quant_finish, rmhmc_quant_dev).
#pragma once
#include "../../include/rmhmc.h"

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <new>

// ---- shape constants of quant.hip.h -------------------------------------------------------------------------------------------------------
#define QUANT_MAX_K 16
#define QUANT_MAX_Q 8
#define QUANT_BINS 256
#define QUANT_THREADS 256   // threads of a workgroup: 4 wavefronts
#define QUANT_LANES 64      // copies of the LDS histogram: one per lane of a wavefront, so that no two lanes of one share a counter
#define QUANT_KEYS 64       // keys a thread holds in registers: the rows of its column in the workgroup's row block
#define QUANT_MAX_TILE 64   // widest column tile

// the column tile of P columns: the smallest power of two that holds them, 64 at the most
inline int32_t quant_tile_width(int32_t P) {
  int32_t tw = 1;
  while (tw < P && tw < QUANT_MAX_TILE) tw *= 2;
  return tw;
}
// rows of a workgroup's block: its 256 / tw row lanes hold QUANT_KEYS rows each
inline int64_t quant_block_rows(int32_t tw) { return (int64_t)(QUANT_THREADS / tw) * QUANT_KEYS; }

// ---- the key --------------------------------------------------------------------------------------------------------------------------------
#define QUANT_SIGN 0x8000000000000000ull
#define QUANT_EXP 0x7ff0000000000000ull

// the key of a finite double (include/rmhmc_quant.h); of any other, a value that quant_key_finite refuses
inline uint64_t quant_key(double x) {
  uint64_t u;
  memcpy(&u, &x, 8);
  if (u == QUANT_SIGN) u = 0;  // -0.0 -> +0.0
  return (u & QUANT_SIGN) ? ~u : (u | QUANT_SIGN);
}
// the keys of the finite doubles lie strictly between those of -inf and +inf
inline bool quant_key_finite(uint64_t key) { return key > ~(QUANT_SIGN | QUANT_EXP) && key < (QUANT_SIGN | QUANT_EXP); }
inline double quant_unkey(uint64_t key) {
  const uint64_t u = (key & QUANT_SIGN) ? (key ^ QUANT_SIGN) : ~key;
  double x;
  memcpy(&x, &u, 8);
  return x;
}
// the digit of round r: key bits 63-8r .. 56-8r
inline int32_t quant_digit(uint64_t key, int32_t round) { return (int32_t)((key >> (56 - 8 * round)) & 255u); }
// whether a key belongs to the target of `prefix` in round r: the top 8r bits agree (round 0: always)
inline bool quant_match(uint64_t key, uint64_t prefix, int32_t round) { return round == 0 || ((key ^ prefix) >> (64 - 8 * round)) == 0; }
// the bits of a prefix below the digits of rounds 0 .. r: they carry the count of the bin chosen in round r, saturated
inline uint64_t quant_carry_mask(int32_t round) { return round >= 7 ? 0 : ((uint64_t)1 << (56 - 8 * round)) - 1; }

// ---- plan -----------------------------------------------------------------------------------------------------------------------------------
inline int quant_plan(const int64_t* m, const double* probs, int32_t Q, int32_t P, int64_t* rank, double* frac) {
  if (!m || !probs || !rank || !frac || P < 1 || Q < 1 || Q > QUANT_MAX_Q) return RMHMC_ERR_INVALID;
  for (int32_t j = 0; j < Q; ++j)
    if (!(probs[j] >= 0.0 && probs[j] <= 1.0)) return RMHMC_ERR_INVALID;
  for (int32_t d = 0; d < P; ++d)
    if (m[d] < 0) return RMHMC_ERR_INVALID;
  for (int32_t j = 0; j < Q; ++j)
    for (int32_t d = 0; d < P; ++d) {
      int64_t lo = -1, hi = -1;
      double g = 0.0;
      if (m[d] > 0) {
        const double h = (double)(m[d] - 1) * probs[j];
        const double fl = floor(h);
        lo = (int64_t)fl;
        if (lo > m[d] - 1) lo = m[d] - 1;  // (q = 1 and m - 1 above 2^53: the product can round up)
        g = h - fl;
        hi = lo + 1 < m[d] - 1 ? lo + 1 : m[d] - 1;
      }
      rank[(size_t)(2 * j) * P + d] = lo;
      rank[(size_t)(2 * j + 1) * P + d] = hi;
      frac[(size_t)j * P + d] = g;
    }
  return RMHMC_OK;
}

// ---- one round ------------------------------------------------------------------------------------------------------------------------------
// rmhmc_quant_step: see the header.  Works on copies and writes prefix and rank only when every target passed.
inline int quant_step(const double* const* hists, int32_t k_parts, int32_t P, int32_t K, int32_t round, uint64_t* prefix, int64_t* rank) {
  if (!hists || !prefix || !rank || k_parts < 1 || P < 1 || K < 1 || K > QUANT_MAX_K || round < 0 || round > 7) return RMHMC_ERR_INVALID;
  for (int32_t i = 0; i < k_parts; ++i)
    if (!hists[i]) return RMHMC_ERR_INVALID;
  const size_t len = (size_t)K * P;
  uint64_t* np = new (std::nothrow) uint64_t[len];
  int64_t* nr = new (std::nothrow) int64_t[len];
  int rc = (np && nr) ? RMHMC_OK : RMHMC_ERR_NOMEM;
  const uint64_t below = quant_carry_mask(round);                  // what this round leaves under its digit
  const uint64_t carried = round ? quant_carry_mask(round - 1) : 0;  // what the previous round left under its own
  for (size_t t = 0; rc == RMHMC_OK && t < len; ++t) {
    np[t] = prefix[t];
    nr[t] = rank[t];
    if (rank[t] < 0) continue;
    const size_t d = t % P, kh = round ? t / P : 0;
    uint64_t c[QUANT_BINS] = {0}, total = 0;
    for (int b = 0; b < QUANT_BINS; ++b) {
      double s = 0.0;
      for (int32_t i = 0; i < k_parts; ++i) s += hists[i][(kh * P + d) * QUANT_BINS + b];
      if (!(s >= 0.0 && s < 9007199254740992.0 && s == floor(s))) rc = RMHMC_ERR_INVALID;
      else { c[b] = (uint64_t)s; total += c[b]; }
    }
    if (rc != RMHMC_OK) break;
    if (total <= (uint64_t)rank[t]) rc = RMHMC_ERR_INVALID;
    if (round) {
      const uint64_t want = prefix[t] & carried;
      if (want < carried ? total != want : total < carried) rc = RMHMC_ERR_INVALID;
    }
    if (rc != RMHMC_OK) break;
    uint64_t cum = 0;
    int b = 0;
    while (cum + c[b] <= (uint64_t)rank[t]) cum += c[b++];
    nr[t] = rank[t] - (int64_t)cum;
    const uint64_t digits = round ? prefix[t] & ~carried : 0;
    np[t] = digits | ((uint64_t)b << (56 - 8 * round)) | (c[b] < below ? c[b] : below);
  }
  if (rc == RMHMC_OK)
    for (size_t t = 0; t < len; ++t) { prefix[t] = np[t]; rank[t] = nr[t]; }
  delete[] np;
  delete[] nr;
  return rc;
}

// ---- finish ---------------------------------------------------------------------------------------------------------------------------------
inline int quant_finish(const uint64_t* prefix, const double* frac, const int64_t* m, int32_t Q, int32_t P, double* quant) {
  if (!prefix || !frac || !m || !quant || P < 1 || Q < 1 || Q > QUANT_MAX_Q) return RMHMC_ERR_INVALID;
  for (int32_t j = 0; j < Q; ++j)
    for (int32_t d = 0; d < P; ++d) {
      double v = NAN;
      if (m[d] > 0) {
        const double lo = quant_unkey(prefix[(size_t)(2 * j) * P + d]), hi = quant_unkey(prefix[(size_t)(2 * j + 1) * P + d]);
        const double g = frac[(size_t)j * P + d];
        v = g == 0.0 ? lo : fma(g, hi - lo, lo);  // (fma: one rounding, whatever the compiler contracts)
      }
      quant[(size_t)j * P + d] = v;
    }
  return RMHMC_OK;
}

// the finite values per dimension: the totals of a (merged) round-0 histogram [1][P][256]
inline void quant_totals(const double* hist0, int32_t P, int64_t* m) {
  for (int32_t d = 0; d < P; ++d) {
    double s = 0.0;
    for (int b = 0; b < QUANT_BINS; ++b) s += hist0[(size_t)d * QUANT_BINS + b];
    m[d] = (int64_t)s;
  }
}
