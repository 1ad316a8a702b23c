// smc.hip.h — the per-stage device work of adaptive sequential Monte Carlo (include/rmhmc_smc.h).  The stepping is
// that of ais.hip.h, unchanged; what is here is small next to it: the conditional ESS of candidate steps, the reweighting, and systematic
// resampling on integers.
//
// Conditional ESS (the partial of include/rmhmc_smc.h), three kernels (maxima, sums, finish: as the weights of ais.hip.h, but every
// quantity is scaled by its own maximum), no atomics, every order fixed by n alone.  JT is the number of candidates
// the instantiation carries (the caller pads its J with copies of the last); NQ = 1 + 2 JT quantities, numbered 0: lw, 1 + 2 j: lw + t_j, 2 + 2 j: lw + 2 t_j, which is the order of the pairs of the partial.
//   k_smc_cess_max<JT>   grid: blocks of ais_plan x 256 threads.  One read of lw and l per entry; the block's maximum of every quantity
//                        -> blk [nblocks][NQ]
//   k_smc_cess_sums<JT>  the same grid.  Every block first takes the global maxima from blk (the same values in each); thread t adds the
//                        NQ terms exp(x - a) of its entries t, t + 256, ... into sum_pairs (sums.hip.h) held in registers; the pairs of the
//                        256 threads are added in thread order, eight quantities at a time through LDS -> sums [nblocks][NQ][2]
//   k_smc_cess_fin       thread q: quantity q over the blocks in block order -> partial [2 + 4 J]
// A quantity whose maximum is -inf has every term 0 and is not evaluated; no index depends on the data.
//
// Resampling.  k_smc_quantise turns log weights into integers q <= 2^40; the inclusive prefix sums C of q are block scans
// (k_smc_scan_blocks: blocks of smc_scan_plan, 256 threads of 4 consecutive entries) plus the exclusive scan of the block totals
// (k_smc_scan_offsets, one block), exact in uint64 whatever the order; k_smc_ancestors is one binary search per offspring on
// C_i (n 2^32) > (j 2^32 + U) Q, both sides as (hi, lo) pairs of 64-bit words; k_smc_gather copies the positions.
#pragma once
#include <hip/hip_runtime.h>

#include "smc.h"
#include "sums.hip.h"  // sum_pair, block_rows, SUM_NEG_INF

#pragma clang fp contract(off)

struct SmcDeltas { double d[RMHMC_SMC_MAX_J]; };

__device__ __forceinline__ double smc_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double u = __shfl_xor(v, o);
    v = u > v ? u : v;
  }
  return v;
}

template <int JT>
__global__ __launch_bounds__(256) void k_smc_cess_max(const double* __restrict__ lw, const double* __restrict__ ll, size_t n, size_t per_block,
                                                      SmcDeltas dl, double* __restrict__ blk) {
  constexpr int NQ = 1 + 2 * JT;
  __shared__ double r[4][NQ];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const block_range rg = block_rows(blockIdx.x, per_block, n);
  double a[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) a[q] = SUM_NEG_INF;
  for (size_t i = rg.begin + tid; i < rg.end; i += 256) {
    const double x = lw[i];
    if (x != x) continue;
    const double l = ll[i];
    a[0] = x > a[0] ? x : a[0];
    if (!isfinite(l)) continue;
#pragma unroll
    for (int j = 0; j < JT; ++j) {
      const double t = dl.d[j] * l;
      const double x1 = x + t, x2 = x + 2.0 * t;
      a[1 + 2 * j] = x1 > a[1 + 2 * j] ? x1 : a[1 + 2 * j];
      a[2 + 2 * j] = x2 > a[2 + 2 * j] ? x2 : a[2 + 2 * j];
    }
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const double m = smc_wave_max(a[q]);
    if (lane == 0) r[wv][q] = m;
  }
  __syncthreads();
  if (tid < NQ) {
    double m = r[0][tid];
    for (int w = 1; w < 4; ++w) m = r[w][tid] > m ? r[w][tid] : m;
    blk[(size_t)blockIdx.x * NQ + tid] = m;
  }
}

#define SMC_CESS_CHUNK 8
template <int JT>
__global__ __launch_bounds__(256) void k_smc_cess_sums(const double* __restrict__ lw, const double* __restrict__ ll, size_t n, size_t per_block,
                                                       SmcDeltas dl, const double* __restrict__ blk, int nblocks, double* __restrict__ sums) {
  constexpr int NQ = 1 + 2 * JT;
  __shared__ double amax[NQ];
  __shared__ double r_s[SMC_CESS_CHUNK][257], r_e[SMC_CESS_CHUNK][257];  // (257: the summing threads read one column each)
  const int tid = threadIdx.x;
  if (tid < NQ) {
    double m = SUM_NEG_INF;
    for (int b = 0; b < nblocks; ++b) m = blk[(size_t)b * NQ + tid] > m ? blk[(size_t)b * NQ + tid] : m;
    amax[tid] = m;
  }
  __syncthreads();
  const block_range rg = block_rows(blockIdx.x, per_block, n);
  sum_pair S[NQ] = {};
  for (size_t i = rg.begin + tid; i < rg.end; i += 256) {
    const double x = lw[i];
    if (x != x) continue;
    const double l = ll[i];
    if (amax[0] > SUM_NEG_INF) S[0].add(exp(x - amax[0]));
    if (!isfinite(l)) continue;
#pragma unroll
    for (int j = 0; j < JT; ++j) {
      const double t = dl.d[j] * l;
      const double x1 = x + t, x2 = x + 2.0 * t;
      const double a1 = amax[1 + 2 * j], a2 = amax[2 + 2 * j];
      if (a1 > SUM_NEG_INF) S[1 + 2 * j].add(exp(x1 - a1));
      if (a2 > SUM_NEG_INF) S[2 + 2 * j].add(exp(x2 - a2));
    }
  }
#pragma unroll
  for (int q0 = 0; q0 < NQ; q0 += SMC_CESS_CHUNK) {
#pragma unroll
    for (int u = 0; u < SMC_CESS_CHUNK; ++u)
      if (q0 + u < NQ) { r_s[u][tid] = S[q0 + u].s; r_e[u][tid] = S[q0 + u].e; }
    __syncthreads();
    if (tid < SMC_CESS_CHUNK && q0 + tid < NQ) {
      sum_pair s = {r_s[tid][0], r_e[tid][0]};
      for (int t = 1; t < 256; ++t) s.add(sum_pair{r_s[tid][t], r_e[tid][t]});
      double* out = sums + 2 * ((size_t)blockIdx.x * NQ + q0 + tid);
      out[0] = s.s; out[1] = s.e;
    }
    __syncthreads();
  }
}

// nq: the quantities the kernels carried (the stride of blk and sums); nq_out = 1 + 2 J <= nq: those the partial keeps
__global__ __launch_bounds__(128) void k_smc_cess_fin(const double* __restrict__ blk, const double* __restrict__ sums, int nblocks, int nq, int nq_out,
                                                      double* __restrict__ partial) {
  const int q = threadIdx.x;
  if (q >= nq_out) return;
  double a = SUM_NEG_INF;
  sum_pair s = {};
  for (int b = 0; b < nblocks; ++b) {
    const double m = blk[(size_t)b * nq + q];
    a = m > a ? m : a;
    const double* in = sums + 2 * ((size_t)b * nq + q);
    s.add(sum_pair{in[0], in[1]});
  }
  partial[2 * q] = a;
  partial[2 * q + 1] = s.value();
}

__global__ __launch_bounds__(256) void k_smc_reweight(double* __restrict__ lw, const double* __restrict__ ll, size_t n, double delta) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double x = lw[i], l = ll[i];
  if (x != x) return;  // (NaN stays)
  lw[i] = isfinite(l) ? x + delta * l : SUM_NEG_INF;
}

__global__ __launch_bounds__(256) void k_smc_quantise(const double* __restrict__ lw, size_t n, double a, unsigned long long* __restrict__ q) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double x = lw[i];
  unsigned long long v = 0ull;
  if (x == x && x > SUM_NEG_INF) {
    const double dx = x - a;  // (a = -inf with a finite x: +inf, and the weight is the full one)
    v = (unsigned long long)floor(0x1p40 * exp(dx < 0.0 ? dx : 0.0));
  }
  q[i] = v;
}

// inclusive scan of the block's 256 x 4 values in place (x: the thread's four consecutive entries); returns the block's total
__device__ __forceinline__ unsigned long long smc_block_scan(unsigned long long x[SMC_SCAN_ITEMS], int tid, unsigned long long* ws /* [4], LDS */) {
  const int wv = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int u = 1; u < SMC_SCAN_ITEMS; ++u) x[u] += x[u - 1];
  const unsigned long long own = x[SMC_SCAN_ITEMS - 1];
  unsigned long long inc = own;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long up = __shfl_up(inc, o);
    if (lane >= o) inc += up;
  }
  if (lane == 63) ws[wv] = inc;
  __syncthreads();
  unsigned long long before = inc - own, total = 0ull;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    if (w < wv) before += ws[w];
    total += ws[w];
  }
#pragma unroll
  for (int u = 0; u < SMC_SCAN_ITEMS; ++u) x[u] += before;
  return total;
}

// q [n] -> C [n]: the prefix sums within each block of SMC_SCAN_BLOCK entries; blk_sum [nblocks]: the blocks' totals; blk_bad [nblocks]:
// whether an entry of the block is above 2^40
__global__ __launch_bounds__(256) void k_smc_scan_blocks(const unsigned long long* __restrict__ q, size_t n, unsigned long long* __restrict__ C,
                                                         unsigned long long* __restrict__ blk_sum, unsigned long long* __restrict__ blk_bad) {
  __shared__ unsigned long long ws[4];
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * SMC_SCAN_BLOCK + (size_t)tid * SMC_SCAN_ITEMS;
  unsigned long long x[SMC_SCAN_ITEMS];
  int bad = 0;
#pragma unroll
  for (int u = 0; u < SMC_SCAN_ITEMS; ++u) {
    x[u] = base + u < n ? q[base + u] : 0ull;
    bad |= x[u] > (1ull << RMHMC_SMC_QBITS);
  }
  bad = __syncthreads_or(bad);
  if (bad) {  // (the sums could overflow: nothing of this block is used, the call refuses)
#pragma unroll
    for (int u = 0; u < SMC_SCAN_ITEMS; ++u) x[u] = 0ull;
  }
  const unsigned long long total = smc_block_scan(x, tid, ws);
#pragma unroll
  for (int u = 0; u < SMC_SCAN_ITEMS; ++u)
    if (base + u < n) C[base + u] = x[u];
  if (tid == 0) { blk_sum[blockIdx.x] = total; blk_bad[blockIdx.x] = bad ? 1ull : 0ull; }
}

// one block: blk_sum [nblocks <= SMC_SCAN_BLOCK] -> off [nblocks]: the sum of the blocks before; head [2] = (Q, the number of bad blocks)
__global__ __launch_bounds__(256) void k_smc_scan_offsets(const unsigned long long* __restrict__ blk_sum, const unsigned long long* __restrict__ blk_bad,
                                                          int nblocks, unsigned long long* __restrict__ off, unsigned long long* __restrict__ head) {
  __shared__ unsigned long long ws[4];
  const int tid = threadIdx.x;
  const int base = tid * SMC_SCAN_ITEMS;
  unsigned long long x[SMC_SCAN_ITEMS], own[SMC_SCAN_ITEMS], b[SMC_SCAN_ITEMS];
#pragma unroll
  for (int u = 0; u < SMC_SCAN_ITEMS; ++u) {
    own[u] = x[u] = base + u < nblocks ? blk_sum[base + u] : 0ull;
    b[u] = base + u < nblocks ? blk_bad[base + u] : 0ull;
  }
  const unsigned long long total = smc_block_scan(x, tid, ws);
#pragma unroll
  for (int u = 0; u < SMC_SCAN_ITEMS; ++u)
    if (base + u < nblocks) off[base + u] = x[u] - own[u];
  __syncthreads();  // (ws is used again)
  const unsigned long long nbad = smc_block_scan(b, tid, ws);
  if (tid == 0) { head[0] = total; head[1] = nbad; }
}

// a b > c d, every factor below 2^64 and every product below 2^128
__device__ __forceinline__ bool smc_prod_gt(unsigned long long a, unsigned long long b, unsigned long long c, unsigned long long d) {
  const unsigned long long lh = __umul64hi(a, b), ll_ = a * b, rh = __umul64hi(c, d), rl = c * d;
  return lh > rh || (lh == rh && ll_ > rl);
}

// anc [j] = min { i : C_i (n 2^32) > (j 2^32 + U) Q }, C_i = C [i] + off [i / SMC_SCAN_BLOCK]; Q > 0, so i = n - 1 satisfies it
__global__ __launch_bounds__(256) void k_smc_ancestors(const unsigned long long* __restrict__ C, const unsigned long long* __restrict__ off, size_t n,
                                                       unsigned int U, unsigned long long Q, int* __restrict__ anc) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const unsigned long long n32 = (unsigned long long)n << 32, pos = ((unsigned long long)j << 32) | (unsigned long long)U;
  size_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const size_t mid = lo + (hi - lo) / 2;
    const unsigned long long c = C[mid] + off[mid / SMC_SCAN_BLOCK];
    if (smc_prod_gt(c, n32, pos, Q)) hi = mid;
    else lo = mid + 1;
  }
  anc[j] = (int)lo;
}

// dst [j][0 .. ld) = src [anc [j]][0 .. ld): different buffers
__global__ __launch_bounds__(64) void k_smc_gather(const double* __restrict__ src, double* __restrict__ dst, const int* __restrict__ anc, int ld) {
  const size_t j = blockIdx.x, i = (size_t)anc[j];
  for (int d = threadIdx.x; d < ld; d += 64) dst[j * ld + d] = src[i * ld + d];
}
