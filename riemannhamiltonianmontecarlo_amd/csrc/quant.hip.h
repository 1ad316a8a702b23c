// Posterior quantiles (include/rmhmc_quant.h): the histogram partial of one round of the radix select from samples [N][P] in device memory.
#pragma once
#include <hip/hip_runtime.h>

#include "quant.h"  // QUANT_THREADS, QUANT_LANES, QUANT_KEYS, the key

#define QUANT_LDS_WORDS (QUANT_BINS * QUANT_LANES)                  // one histogram: 64 KiB
#define QUANT_LDS_BYTES (QUANT_LDS_WORDS * 4 + 16)                  // ... and the three match flags; two workgroups share a CU

// k_quant_hist: a streaming integer histogram.  grid (row blocks, column tiles of TW) x 256 threads; thread = (column dl = tid % TW, row
// lane g = tid / TW of G = 256 / TW) reads rows g, g + G, ... of its column of the block's G * QUANT_KEYS rows ONCE - a wavefront reads
// min(TW, 64) consecutive doubles of a row, as k_diag_acov does - and keeps their keys in registers (QUANT_KEYS x 64 bits, with one bit
// each for "finite and inside the tensor").  It then walks the Kh targets over those registers; the column of a thread is fixed, so the
// prefix of (target, column) is one register pair and a value that matches no prefix costs a masked compare.
//
// LDS holds ONE histogram at a time, as h[bin][lane]: every lane of a wavefront owns a copy of its column's 256 counters, so the lanes of
// a wavefront never meet in a counter, whatever the data (rounds 0 and 1 look at the sign and the exponent: a posterior column falls into
// one or two bins, and one counter per column would serialise every wavefront that holds a column more than once), and lane is the
// bank, so equal bins do not conflict either.  The four wavefronts of the workgroup share the copies through ds_add_u32.  A target that
// no thread of the workgroup matched (most of them from round 2 on) is voted away through an LDS flag and costs no pass over the
// histogram; otherwise the workgroup scans it with 16-byte reads, zeroes what it found for the next target, adds up the 64 / TW copies of a
// column across lanes, and adds the non-zero sums to the global counters [Kh][P][256] with 64-bit integer atomics: integer addition is
// associative, so the result does not depend on the order in which workgroups arrive (include/rmhmc_quant.h).
//
// rep [K][P]: the first target of the column with the same top 8r prefix bits.  Only such a target is counted; k_quant_out copies its
// counters to the others (the lo and hi ranks of a quantile, and often all quantiles of a column, share their leading digits).
template <int TW>
__global__ __launch_bounds__(QUANT_THREADS, 2) void k_quant_hist(const double* __restrict__ samples, long long N, int P, int round, int Kh,
                                                                const unsigned long long* __restrict__ prefix,
                                                                const signed char* __restrict__ rep, unsigned long long* __restrict__ ghist) {
  extern __shared__ __attribute__((aligned(16))) unsigned int qh_lds[];
  constexpr int G = QUANT_THREADS / TW;
  static_assert(QUANT_KEYS == 64 && QUANT_LANES == 64 && QUANT_THREADS == 256, "one validity bit per key, one histogram copy per lane");
  const int tid = threadIdx.x, dl = tid % TW, g = tid / TW, slot = tid & (QUANT_LANES - 1);
  const long long col = (long long)blockIdx.y * TW + dl;
  const bool cvalid = col < P;
  unsigned int* h = qh_lds;
  unsigned int* flag = qh_lds + QUANT_LDS_WORDS;
  uint4* h4 = (uint4*)qh_lds;
  for (int i = tid; i < QUANT_LDS_WORDS / 4; i += QUANT_THREADS) h4[i] = make_uint4(0u, 0u, 0u, 0u);
  if (tid < 3) flag[tid] = 0u;

  unsigned long long keys[QUANT_KEYS];
  unsigned long long valid = 0ull;
  const long long r0 = (long long)blockIdx.x * (G * QUANT_KEYS) + g;
  // every load is issued whether its row exists or not (a row past the end reads element 0): no branch, so the 64 loads of a thread are in
  // flight together; which of them count is one mask worked out from the number of rows, not 64 comparisons kept until the data is there
  long long mine_rows = cvalid ? (N - r0 + G - 1) / G : 0;   // rows r0, r0 + G, ... below N
  mine_rows = mine_rows < 0 ? 0 : mine_rows > QUANT_KEYS ? QUANT_KEYS : mine_rows;
  const int nrows = (int)mine_rows;
#pragma unroll
  for (int i = 0; i < QUANT_KEYS; ++i) {
    const long long r = r0 + (long long)i * G;
    unsigned long long u = (unsigned long long)__double_as_longlong(samples[i < nrows ? (size_t)r * P + col : (size_t)0]);
    if (u == QUANT_SIGN) u = 0ull;
    u = (u & QUANT_SIGN) ? ~u : (u | QUANT_SIGN);
    if (u > ~(QUANT_SIGN | QUANT_EXP) && u < (QUANT_SIGN | QUANT_EXP)) valid |= 1ull << i;
    keys[i] = u;
  }
  valid &= nrows >= 64 ? ~0ull : (1ull << nrows) - 1ull;
  __syncthreads();

  const int dshift = 56 - 8 * round;
  const unsigned long long top = round ? ~0ull << (64 - 8 * round) : 0ull;  // the prefix bits of the round
  for (int k = 0; k < Kh; ++k) {
    // flag[k % 3] is this target's; the next one's was last read two targets ago, before the barrier every thread has since passed
    if (tid == 0) flag[(k + 1) % 3] = 0u;
    unsigned long long pk = 0ull;
    bool mine = cvalid && valid != 0ull;
    if (round && cvalid) {
      pk = prefix[(size_t)k * P + col];
      mine = mine && rep[(size_t)k * P + col] == k;
    }
    if (mine) {
      // which of the thread's keys belong to the target: a mask worked out without a branch (two xors, two ands and a compare per
      // key), so that a value that matches nothing costs that and no more, and a wavefront none of whose lanes has a match (most of
      // them from round 3 on) skips the adds in one branch
      unsigned long long hit = 0ull;
#pragma unroll
      for (int i = 0; i < QUANT_KEYS; ++i) hit |= (unsigned long long)(((keys[i] ^ pk) & top) == 0ull) << i;
      hit &= valid;
      if (hit) {
#pragma unroll
        for (int i = 0; i < QUANT_KEYS; ++i)
          if ((hit >> i) & 1ull) atomicAdd(&h[(int)((keys[i] >> dshift) & 255ull) * QUANT_LANES + slot], 1u);
        flag[k % 3] = 1u;
      }
    }
    __syncthreads();
    if (flag[k % 3] == 0u) continue;  // (the same for every thread of the workgroup)
    // the scan: uint4 j = tid + 256 i holds bin j / 16 = tid / 16 + 16 i, lanes 4 (tid % 16) .. + 3
    const int l4 = tid & 15;
#pragma unroll 4
    for (int i = 0; i < QUANT_LDS_WORDS / 4 / QUANT_THREADS; ++i) {
      const int j = tid + QUANT_THREADS * i;
      const uint4 v = h4[j];
      if (v.x | v.y | v.z | v.w) h4[j] = make_uint4(0u, 0u, 0u, 0u);
      unsigned int c[4] = {v.x, v.y, v.z, v.w};
      // lane s of the histogram counted column s % TW: add up the copies of a column
      if (TW == 2) { c[0] += c[2]; c[1] += c[3]; }
      if (TW == 1) c[0] += c[1] + c[2] + c[3];
#pragma unroll
      for (int m = (TW >= 4 ? TW / 4 : 1); m < 16; m *= 2)
#pragma unroll
        for (int e = 0; e < (TW >= 4 ? 4 : TW); ++e) c[e] += __shfl_xor(c[e], m);
      if (l4 < (TW >= 4 ? TW / 4 : 1)) {
        const int bin = j >> 4;
#pragma unroll
        for (int e = 0; e < (TW >= 4 ? 4 : TW); ++e) {
          const long long gc = (long long)blockIdx.y * TW + 4 * l4 + e;
          if (c[e] && gc < P) atomicAdd(&ghist[((size_t)k * P + gc) * QUANT_BINS + bin], (unsigned long long)c[e]);
        }
      }
    }
    __syncthreads();  // the histogram is zero again before the next target adds to it
  }
}

// the 64-bit counters [Kh][P][256] -> the partial, doubles; a target takes the counters of its representative (rep NULL: its own)
__global__ __launch_bounds__(256) void k_quant_out(const unsigned long long* __restrict__ ghist, const signed char* __restrict__ rep, int P,
                                                   size_t total, double* __restrict__ hist) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= total) return;
  const size_t b = i % QUANT_BINS, t = i / QUANT_BINS, d = t % P;
  const size_t k = rep ? (size_t)rep[t] : t / P;
  hist[i] = (double)ghist[(k * P + d) * QUANT_BINS + b];
}
