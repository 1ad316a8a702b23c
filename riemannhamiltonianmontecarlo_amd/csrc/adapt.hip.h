// Pooled mean and covariance of samples [N][P] in device memory (include/rmhmc_adapt.h): the partial of adapt.h.  N = n S rows of a
// *_sample_to buffer [n][S][P], P <= COV_MAX_P.
//
// Two passes, four kernels, no atomics; every sum has a fixed order that depends on (N, P) alone, so a call repeats bit for bit.
//   k_cov_sums    grid: row blocks of cov_plan_sums x 256 threads.  A wavefront takes the rows wv, wv + 4, ... of its block, lane l the
//                 columns l, l + 64, ...: a row with a non-finite entry (wave_row_finite) is flagged in valid[] and skipped, the
//                 others are added to the lane's column sums, each a sum_pair of sums.hip.h.  The four wavefronts meet in LDS in the
//                 order 0..3.  Output: blk [nblocks][3][P], rows (sum, error, rows used in entry 0).
//   k_cov_mean    one workgroup: the blocks added in block order (pairs again); rows 0 and 1 of the partial, and the centre as a pair
//                 (hi = row 1, lo) with hi + lo the mean to about twice the precision of a double.
//   k_cov_xtx     grid: (pairs I <= J of 16-column tiles, row blocks of cov_plan) x one wavefront.  Xc' Xc of the block's rows on
//                 v_mfma_f64_16x16x4_f64, four sample rows per instruction: lane l holds A[i = l & 15][k = l >> 4] = xc[r0 + k][16 I + i]
//                 and B[k][j = l & 15] = xc[r0 + k][16 J + j], each read straight from global memory (16 consecutive doubles of a row
//                 per quarter wavefront: full 128-byte lines), centred as (x - hi) - lo, and zero for a row that is flagged, past the end,
//                 or a column >= P.  Exact zeros add nothing, so padding never shows.  The 16 x 16 result (row (l >> 4) + 4 e, column
//                 l & 15 in element e) goes to the workgroup's own tile of scr [nblocks][P][P].
//   k_cov_reduce  one thread per entry i <= j: the blocks added in block order, written to (i, j) and (j, i) of the partial: C is
//                 symmetric to the bit.
// The second pass centres about the mean the first has summed; it is never E[xx'] - mean mean'.  Why the pair: with |mean| = 1e8 and
// unit spread the centre of a plain double is off by up to 1e-8, which adds N 1e-16 to every entry of C - as much as the rounding of
// the N products themselves for small N.  The tile operands come from global memory without an LDS stage: a tile pair reads each of
// its rows once, and the rows of a column tile are shared by the pairs of one row block through the L2.
#pragma once
#include <hip/hip_runtime.h>

#include "adapt.h"     // COV_MAX_P, the row blocks
#include "sums.hip.h"  // sum_pair, sum_finite, block_rows, wave_row_finite, d4

static_assert(COV_MAX_P == 256, "wave_row_finite checks 256 columns");

__global__ __launch_bounds__(256) void k_cov_sums(const double* __restrict__ x, size_t N, int P, size_t rows_per_block,
                                                  unsigned char* __restrict__ valid, double* __restrict__ blk) {
  __shared__ sum_pair red[4][COV_MAX_P];
  __shared__ double red_m[4];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const block_range rows = block_rows(blockIdx.x, rows_per_block, N);
  sum_pair sum[4] = {};
  double used = 0.0;
  for (size_t r = rows.begin + wv; r < rows.end; r += 4) {
    double v[4];
    const bool ok = wave_row_finite(x + r * (size_t)P, P, lane, v);
    if (lane == 0) valid[r] = ok ? 1 : 0;
    if (ok) {
      used += 1.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) sum[q].add(v[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) red[wv][lane + 64 * q] = sum[q];
  if (lane == 0) red_m[wv] = used;
  __syncthreads();
  if (tid < P) {
    sum_pair t = red[0][tid];
    for (int w = 1; w < 4; ++w) t.add(red[w][tid]);
    double* out = blk + (size_t)blockIdx.x * 3 * (size_t)P;
    out[tid] = t.s;
    out[P + tid] = t.e;
    if (tid == 0) out[2 * (size_t)P] = ((red_m[0] + red_m[1]) + red_m[2]) + red_m[3];
  }
}

// blk [nblocks][3][P] -> rows 0 and 1 of the partial and the centre ctr [2][P] = (hi, lo)
__global__ __launch_bounds__(256) void k_cov_mean(const double* __restrict__ blk, size_t nblocks, int P, double* __restrict__ partial,
                                                  double* __restrict__ ctr) {
  const int c = threadIdx.x;
  if (c >= P) return;
  const size_t p = (size_t)P;
  sum_pair t = {};
  double m = 0.0;
  for (size_t b = 0; b < nblocks; ++b) {
    const double* in = blk + b * 3 * p;
    t.add(sum_pair{in[c], in[p + c]});
    m += in[2 * p];
  }
  double hi = 0.0, lo = 0.0;
  if (m > 0.0) {
    const double sh = t.value(), sl = t.e - (sh - t.s);  // (|e| <= |s| ulp-wise: fast two-sum)
    hi = sh / m;
    lo = (fma(-hi, m, sh) + sl) / m;
    if (!sum_finite(hi) || !sum_finite(lo)) lo = 0.0;  // (the sum has overflowed: hi says so)
  }
  partial[c] = m;
  partial[p + c] = hi;
  ctr[c] = hi;
  ctr[p + c] = lo;
}

__global__ __launch_bounds__(64) void k_cov_xtx(const double* __restrict__ x, size_t N, int P, size_t rows_per_block,
                                                const unsigned char* __restrict__ valid, const double* __restrict__ ctr,
                                                double* __restrict__ scr) {
  const int lane = threadIdx.x, a = lane & 15, k = lane >> 4;
  int I = 0, J = (int)blockIdx.x;
  const int nt = (P + 15) >> 4;
  while (J >= nt - I) { J -= nt - I; ++I; }  // pair number -> (I, J), I <= J: row I of the triangle has nt - I pairs
  J += I;
  const int ca = 16 * I + a, cb = 16 * J + a;
  const bool in_a = ca < P, in_b = cb < P;
  const size_t p = (size_t)P;
  const double hia = in_a ? ctr[ca] : 0.0, loa = in_a ? ctr[p + ca] : 0.0;
  const double hib = in_b ? ctr[cb] : 0.0, lob = in_b ? ctr[p + cb] : 0.0;
  const block_range rows = block_rows(blockIdx.y, rows_per_block, N);  // (begin a multiple of 4)
  const size_t r_begin = rows.begin, r_end = rows.end;
  d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
  const long long nsteps = r_end > r_begin ? (long long)((r_end - r_begin + 3) / 4) : 0;
  // (branch-free, so that the loads of several steps are in flight: a lane without an operand reads row r_end - 1 or column 0 of
  // the block, which exist, and selects zero)
  const size_t cca = in_a ? (size_t)ca : 0, ccb = in_b ? (size_t)cb : 0;
  auto step = [&](long long it) {
    const size_t r = r_begin + 4 * (size_t)it + (size_t)k;
    const size_t rc = r < r_end ? r : r_end - 1;
    const bool ok = r < r_end && valid[rc] != 0;
    const double xa = x[rc * p + cca], xb = x[rc * p + ccb];
    const double va = (ok && in_a) ? (xa - hia) - loa : 0.0;
    const double vb = (ok && in_b) ? (xb - hib) - lob : 0.0;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(va, vb, acc, 0, 0, 0);
  };
  // (unrolled by hand: the MFMA is a convergent operation, which a loop of unknown length is not unrolled around)
  long long it = 0;
  for (; it + 4 <= nsteps; it += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) step(it + u);
  }
  for (; it < nsteps; ++it) step(it);
  double* out = scr + (size_t)blockIdx.y * p * p;
  if (in_b) {
#pragma unroll
    for (int el = 0; el < 4; ++el) {
      const int ri = 16 * I + k + 4 * el;
      if (ri < P) out[(size_t)ri * p + (size_t)cb] = acc[el];
    }
  }
}

__global__ __launch_bounds__(256) void k_cov_reduce(const double* __restrict__ scr, size_t nblocks, int P, double* __restrict__ partial) {
  const size_t p = (size_t)P;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= p * p) return;
  const size_t i = idx / p, j = idx % p;
  if (i > j) return;
  double sum = 0.0;
#pragma unroll 8
  for (size_t b = 0; b < nblocks; ++b) sum += scr[b * p * p + idx];
  partial[(2 + i) * p + j] = sum;
  partial[(2 + j) * p + i] = sum;
}
