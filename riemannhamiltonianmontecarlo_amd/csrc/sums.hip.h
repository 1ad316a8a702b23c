// sums.hip.h — what the summary kernels share (adapt, ais, smc, pred, loo, diag .hip.h): the compensated sum, the finite test, a block's
// range of rows and a wavefront's validity check of one row.  Nothing here decides an order: every kernel keeps its own.
#pragma once
#include <hip/hip_runtime.h>

typedef double d4 __attribute__((ext_vector_type(4)));  // the accumulator of v_mfma_f64_16x16x4_f64

#define SUM_NEG_INF (-__builtin_huge_val())

// neither NaN nor +-inf
__device__ __forceinline__ bool sum_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// (s, e) <- (s, e) + x with the rounding error of the sum kept in e (Knuth).  The additions are never contracted with a product of the
// caller's, whatever mode the including file is in.
__device__ __forceinline__ void two_sum(double& s, double& e, double x) {
#pragma clang fp contract(off)
  const double t = s + x;
  const double bp = t - s;
  e += (s - (t - bp)) + (x - bp);
  s = t;
}

// an unevaluated sum s + e
struct sum_pair {
  double s, e;
  __device__ __forceinline__ void add(double x) { two_sum(s, e, x); }
  __device__ __forceinline__ void add(const sum_pair& o) {
    two_sum(s, e, o.s);
    e += o.e;
  }
  __device__ __forceinline__ double value() const { return s + e; }
};

// rows [begin, end) of block b where a block takes per_block of n rows
struct block_range { size_t begin, end; };
__device__ __forceinline__ block_range block_rows(size_t b, size_t per_block, size_t n) {
  const size_t begin = b * per_block;
  return {begin, begin + per_block < n ? begin + per_block : n};
}

// A wavefront's check of one row of ncols <= 256 columns: lane l loads the columns l, l + 64, l + 128, l + 192 into v (0.0 past the
// end); true, in every lane, where the whole row is finite.
__device__ __forceinline__ bool wave_row_finite(const double* __restrict__ row, int ncols, int lane, double v[4]) {
  int bad = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = lane + 64 * q;
    v[q] = c < ncols ? row[c] : 0.0;
    bad |= !sum_finite(v[q]);
  }
  return __ballot(bad) == 0ULL;
}
