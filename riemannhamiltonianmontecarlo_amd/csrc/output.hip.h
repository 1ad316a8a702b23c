// Write-out of a sampler call (include/rmhmc_out.h): the one reduction the ESS kernel does not cover.
#pragma once
#include <hip/hip_runtime.h>

// run_mean[s][d] = (sum over the chains c = 0 .. n-1, in that order, of samples[c][s][d]) / n: the run-mean chain of the reference
// driver (main.py:54).  A thread owns one (s, d) = one element i of the S x D block and walks the n blocks, so the sum does not depend
// on the launch geometry; adjacent threads take adjacent d, so a wavefront reads 512 contiguous bytes of every chain.  Memory-bound: the
// samples are read once; the unrolled loads of one thread are independent, only the adds are chained.  A NaN row of one chain (a stopped
// Gibbs chain) makes that row of the result NaN and no other.
__global__ __launch_bounds__(256) void k_run_mean(const double* __restrict__ samples, size_t n, size_t SD, double* __restrict__ run_mean) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= SD) return;
  const double* __restrict__ x = samples + i;
  double sum = 0.0;
#pragma unroll 8
  for (size_t c = 0; c < n; ++c) sum += x[c * SD];
  run_mean[i] = sum / (double)n;
}
