// pred.h — the host half of the posterior predictive probabilities (include/rmhmc_pred.h): the shape of a partial, the merge of two
// partials and the finish, and the plan of the kernels of pred.hip.h (rows per workgroup, draws per block, number of blocks, scratch
// size) as functions of (N, R, D).  No HIP header: plain C++17, so a host compiler alone builds it (tests/helpers/pred_probe.cpp)
// and the library calls the same code (rmhmc_pred_finish, rmhmc_pred_partial_dev).
//
// A partial of R rows is double[4 * R], rows of length R, about the draws used (a draw with a non-finite entry is not used):
//   row 0  m, the number of draws used (an exact integer, in every entry)
//   row 1  S1 = sum over them of p       row 2  S2 = sum of p^2       row 3  SQ = sum of q (-0.0 in every entry without labels)
#pragma once
#include "../../include/rmhmc.h"

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <new>

// ---- shape constants of pred.hip.h -------------------------------------------------------------------------------------------------------
#define PRED_MAX_D 256
#define PRED_WAVE_ROWS 16                  // rows of xnew a wavefront owns: the A operand of v_mfma_f64_16x16x4_f64
#define PRED_WAVES 4                       // wavefronts of a workgroup; all walk the same draws
#define PRED_ROW_TILE (PRED_WAVE_ROWS * PRED_WAVES)   // rows of xnew per workgroup
#define PRED_DRAWS 256                     // the largest draw block while the limits below allow: a constant, so the split depends on (N, R) alone
#define PRED_MAX_BLOCKS 1024               // draw blocks of either pass
#define PRED_SCRATCH_BYTES (64 << 20)      // bound of the records [row tiles][blocks][3][PRED_ROW_TILE] of the main kernel

// MFMA steps (of 4 k each) the main kernel is compiled for, 4 or a multiple of 8: the xnew tile of a wavefront is ksteps doubles per
// lane, held in registers; steps past ceil(D / 4) multiply exact zeros
inline int32_t pred_ksteps(int32_t D) { return D <= 16 ? 4 : (D + 31) / 32 * 8; }

struct pred_plan_t {
  int64_t row_tiles;        // workgroups along R, PRED_ROW_TILE rows each
  int64_t nblocks;          // draw blocks of the main kernel
  int64_t draws_per_block;  // a multiple of 16, the draws of one MFMA tile
  int64_t vblocks;          // draw blocks of the validity pass
  int64_t draws_per_vblock;
  int32_t ksteps;
  // the scratch buffer of a call, in this order (every offset a multiple of 8 bytes):
  int64_t rec_doubles;      // records [row_tiles][nblocks][3][PRED_ROW_TILE]
  int64_t cnt_doubles;      // draws used per block of the validity pass [vblocks]
  int64_t x_doubles;        // xnew [R][D] and tnew [R]
  int64_t valid_bytes;      // one flag per draw [N], rounded up to a multiple of 8
  int64_t scratch_bytes;
};

// The plan of N draws, R rows, D columns (all >= 1, D <= PRED_MAX_D).  The main kernel's blocks: ceil(N / PRED_DRAWS) equal blocks, or
// as many as PRED_MAX_BLOCKS and the scratch bound allow where that is fewer.  The validity pass: the same under PRED_MAX_BLOCKS alone.
inline pred_plan_t pred_plan(int64_t N, int64_t R, int32_t D) {
  pred_plan_t p;
  p.row_tiles = (R + PRED_ROW_TILE - 1) / PRED_ROW_TILE;
  int64_t mb = (int64_t)PRED_SCRATCH_BYTES / (p.row_tiles * 3 * PRED_ROW_TILE * 8);
  mb = mb < 1 ? 1 : mb > PRED_MAX_BLOCKS ? PRED_MAX_BLOCKS : mb;
  int64_t nb = (N + PRED_DRAWS - 1) / PRED_DRAWS;
  if (nb > mb) nb = mb;
  p.draws_per_block = ((N + nb - 1) / nb + 15) / 16 * 16;
  p.nblocks = (N + p.draws_per_block - 1) / p.draws_per_block;
  int64_t vb = (N + PRED_DRAWS - 1) / PRED_DRAWS;
  if (vb > PRED_MAX_BLOCKS) vb = PRED_MAX_BLOCKS;
  p.draws_per_vblock = (N + vb - 1) / vb;
  p.vblocks = (N + p.draws_per_vblock - 1) / p.draws_per_vblock;
  p.ksteps = pred_ksteps(D);
  p.rec_doubles = p.row_tiles * p.nblocks * 3 * PRED_ROW_TILE;
  p.cnt_doubles = p.vblocks;
  p.x_doubles = R * (int64_t)D + R;
  p.valid_bytes = (N + 7) / 8 * 8;
  p.scratch_bytes = 8 * (p.rec_doubles + p.cnt_doubles + p.x_doubles) + p.valid_bytes;
  return p;
}

// ---- the host checks of rmhmc_pred_partial_dev: nullptr, or what is refused ---------------------------------------------------------------
inline const char* pred_check_rows(const double* xnew, const double* tnew, int64_t R, int32_t D) {
  for (int64_t i = 0; i < R * (int64_t)D; ++i)
    if (!std::isfinite(xnew[i])) return "an entry of xnew is not finite";
  if (tnew)
    for (int64_t r = 0; r < R; ++r)
      if (!(tnew[r] == 0.0 || tnew[r] == 1.0)) return "an entry of tnew is neither 0 nor 1";
  return nullptr;
}

// ---- merge and finish --------------------------------------------------------------------------------------------------------------------
// a <- a merged with b (both of R rows): the four rows added, one rounding per entry.  A partial with m = 0 is the identity, to the bit.
inline void pred_merge(double* a, const double* b, int64_t R) {
  if (b[0] == 0.0) return;
  const size_t len = 4 * (size_t)R;
  if (a[0] == 0.0) {
    for (size_t i = 0; i < len; ++i) a[i] = b[i];
    return;
  }
  for (size_t i = 0; i < len; ++i) a[i] += b[i];
}

// rmhmc_pred_finish (include/rmhmc_pred.h): merges the k partials in the order given into `merged` (or a buffer of its own) and
// finishes.  prob = S1 / m; pvar = max(0, S2 / m - prob^2): every term lies in [0, 1], so the subtraction costs an absolute 4 * 2^-53
// and no more (a rounding of S2 / m, of prob twice through the square, and of the difference); lpd = log(SQ / m), -inf for SQ = 0;
// lpd_total = sum of lpd in row order.  m = 0: NaN everywhere.  Without labels row 3 is -0.0 in every entry, which no sum of
// likelihoods is (they start from +0.0 and add q >= +0.0) and which merging keeps (-0.0 + -0.0 = -0.0): lpd is NaN for such an entry.
// Returns RMHMC_OK, RMHMC_ERR_INVALID, RMHMC_ERR_NOMEM.
inline int pred_finish(const double* const* partials, int32_t k, int64_t R, double* merged, double* prob, double* pvar,
                       double* lpd, double* lpd_total, int64_t* draws_used) {
  if (!partials || k < 1 || R < 1) return RMHMC_ERR_INVALID;
  for (int32_t i = 0; i < k; ++i)
    if (!partials[i]) return RMHMC_ERR_INVALID;
  const size_t r = (size_t)R, len = 4 * r;
  double* own = nullptr;
  if (!merged) {
    own = new (std::nothrow) double[len];
    if (!own) return RMHMC_ERR_NOMEM;
    merged = own;
  }
  for (size_t i = 0; i < len; ++i) merged[i] = 0.0;
  for (int32_t i = 0; i < k; ++i) pred_merge(merged, partials[i], R);
  const double m = merged[0];
  double total = 0.0;
  for (size_t i = 0; i < r; ++i) {
    double pr = NAN, pv = NAN, lp = NAN;
    if (m > 0.0) {
      pr = merged[r + i] / m;
      pv = merged[2 * r + i] / m - pr * pr;
      if (pv < 0.0) pv = 0.0;  // (a NaN stays a NaN)
      const double sq = merged[3 * r + i];
      if (!(sq == 0.0 && std::signbit(sq))) lp = log(sq / m);
    }
    if (prob) prob[i] = pr;
    if (pvar) pvar[i] = pv;
    if (lpd) lpd[i] = lp;
    total += lp;
  }
  if (lpd_total) *lpd_total = total;
  if (draws_used) *draws_used = (int64_t)m;
  delete[] own;
  return RMHMC_OK;
}
