// Pooled mean and covariance of samples [N][P] in device memory (include/rmhmc_adapt.h): the partial of adapt.h.  N = n S rows of a
// *_sample_to buffer [n][S][P], P <= COV_MAX_P.
//
// Two passes, four kernels, no atomics; every sum has a fixed order that depends on (N, P) alone, so a call repeats bit for bit.
//   k_cov_sums    grid: row blocks of cov_plan_sums x 256 threads.  A wavefront takes the rows wv, wv + 4, ... of its block, lane l the
//                 columns l, l + 64, ...: a row with a non-finite entry (ballot) is flagged in valid[] and skipped, the others are
//                 added to the lane's column sums, kept as an unevaluated pair (sum, error) by Knuth's two-sum.  The four wavefronts
//                 meet in LDS in the order 0..3.  Output: blk [nblocks][3][P], rows (sum, error, rows used in entry 0).
//   k_cov_mean    one workgroup: the blocks added in block order (two-sum again); rows 0 and 1 of the partial, and the centre as a pair
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

#include "adapt.h"  // COV_MAX_P, the row blocks

typedef double cov_d4 __attribute__((ext_vector_type(4)));

// (s, e) <- (s, e) + x with the rounding error of the sum kept in e (Knuth)
__device__ __forceinline__ void cov_two_sum(double& s, double& e, double x) {
  const double t = s + x;
  const double bp = t - s;
  e += (s - (t - bp)) + (x - bp);
  s = t;
}

__global__ __launch_bounds__(256) void k_cov_sums(const double* __restrict__ x, size_t N, int P, size_t rows_per_block,
                                                  unsigned char* __restrict__ valid, double* __restrict__ blk) {
  __shared__ double red_s[4][COV_MAX_P], red_e[4][COV_MAX_P];
  __shared__ double red_m[4];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const size_t r_begin = (size_t)blockIdx.x * rows_per_block;
  const size_t r_end = r_begin + rows_per_block < N ? r_begin + rows_per_block : N;
  double s[4] = {0.0, 0.0, 0.0, 0.0}, e[4] = {0.0, 0.0, 0.0, 0.0};
  double used = 0.0;
  for (size_t r = r_begin + wv; r < r_end; r += 4) {
    const double* __restrict__ row = x + r * (size_t)P;
    double v[4];
    int bad = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = lane + 64 * q;
      v[q] = c < P ? row[c] : 0.0;
      bad |= !(fabs(v[q]) <= 1.7976931348623157e308);
    }
    const bool ok = __ballot(bad) == 0ULL;
    if (lane == 0) valid[r] = ok ? 1 : 0;
    if (ok) {
      used += 1.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) cov_two_sum(s[q], e[q], v[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    red_s[wv][lane + 64 * q] = s[q];
    red_e[wv][lane + 64 * q] = e[q];
  }
  if (lane == 0) red_m[wv] = used;
  __syncthreads();
  if (tid < P) {
    double ts = red_s[0][tid], te = red_e[0][tid];
    for (int w = 1; w < 4; ++w) {
      cov_two_sum(ts, te, red_s[w][tid]);
      te += red_e[w][tid];
    }
    double* out = blk + (size_t)blockIdx.x * 3 * (size_t)P;
    out[tid] = ts;
    out[P + tid] = te;
    if (tid == 0) out[2 * (size_t)P] = ((red_m[0] + red_m[1]) + red_m[2]) + red_m[3];
  }
}

// blk [nblocks][3][P] -> rows 0 and 1 of the partial and the centre ctr [2][P] = (hi, lo)
__global__ __launch_bounds__(256) void k_cov_mean(const double* __restrict__ blk, size_t nblocks, int P, double* __restrict__ partial,
                                                  double* __restrict__ ctr) {
  const int c = threadIdx.x;
  if (c >= P) return;
  const size_t p = (size_t)P;
  double s = 0.0, e = 0.0, m = 0.0;
  for (size_t b = 0; b < nblocks; ++b) {
    const double* in = blk + b * 3 * p;
    cov_two_sum(s, e, in[c]);
    e += in[p + c];
    m += in[2 * p];
  }
  double hi = 0.0, lo = 0.0;
  if (m > 0.0) {
    const double sh = s + e, sl = e - (sh - s);  // (|e| <= |s| ulp-wise: fast two-sum)
    hi = sh / m;
    lo = (fma(-hi, m, sh) + sl) / m;
    if (!(fabs(hi) <= 1.7976931348623157e308) || !(fabs(lo) <= 1.7976931348623157e308)) lo = 0.0;  // (the sum has overflowed: hi says so)
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
  const size_t r_begin = (size_t)blockIdx.y * rows_per_block;  // (a multiple of 4)
  const size_t r_end = r_begin + rows_per_block < N ? r_begin + rows_per_block : N;
  cov_d4 acc = (cov_d4){0.0, 0.0, 0.0, 0.0};
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
