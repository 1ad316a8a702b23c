// Cross-chain diagnostics (include/rmhmc_diag.h): the partial of diag.h from samples [n][S][P] in device memory.
#pragma once
#include <hip/hip_runtime.h>

#include "diag.h"      // DIAG_CHAINS, DIAG_THREADS, DIAG_R, the LDS image
#include "sums.hip.h"  // sum_finite

// Every chain gives two series per dimension: its first H = S / 2 rows and its last H rows.  k_diag_acov sums, over the series of a
// block of DIAG_CHAINS chains, the raw lag products sum_s x_s x_{s+t} of the centred series for t < T, and counts the series it used.
//
// grid (dimension tiles of TW, chain blocks) x 256 threads; thread = (column dl = tid % TW, lag group g = tid / TW of G = 256 / TW) owns
// NQ sets of 16 lags of column dl, set q starting at tg = 16 (G q + g), for ALL series of the block: 16 NQ accumulators in registers,
// added to in chain order (chain c0, first half, second half, chain c0 + 1, ...), so a block's sums depend on nothing but the samples
// and the constants of diag.h.  NQ = 1 where 16 G lags cover T, else 4: with the tile widths of diag_tile_width 64 G lags cover every
// T <= H (diag.h), so the samples are read once whatever T is, and the sets of a thread are interleaved with those of the other
// groups (16 G apart), which spreads the triangle of the all-lag case evenly over the wavefronts.  No atomics: a block writes its own
// rows of blk [nblocks][2 + T][P] (row 0: series used, row 1: the sum of their means, row 2 + t: the lag sums), and k_diag_reduce adds
// the blocks in block order.
//
// Per series: the 256 threads read the H x TW tile of sample rows (a wavefront reads min(TW, 64) contiguous doubles of a row, where
// k_ess's stride-P walk takes 8 bytes of every 8 P), thread (dl, g) rows g, g + G, ... of its own column, into LDS; the column sums are
// reduced through LDS in the fixed order g = 0 .. G-1, the tile is centred in place (never E[x^2] - E[x]^2), and a column with a
// non-finite value is zeroed instead: it then adds exact zeros to every accumulator and is not counted (its mean is recorded as NaN
// for k_diag_m2).  The tile is followed by zero rows, so the lag loop needs no bounds: x_{s+t} beyond the series is 0 and adds nothing.
//
// The lag loop is register-blocked, or it would be LDS-bound (one ds_read_b64 per fp64 FMA against 4 FMA wave-instructions per LDS
// read the CU can retire): per step of 16 rows a thread reads its 16 x_s and a window of 31 x_{s+t} once, 47 LDS reads, for 256 FMAs.
// A lag set stops at s + tg >= H, so the all-lag case costs the triangle, not the square.  The tile is kept to half the LDS where a
// narrower one fits (diag_tile_width), so that two workgroups share a CU and one loads while the other multiplies; 242 VGPRs at NQ = 4
// allow that.  LDS row r lives at r + r / 16: groups 16 rows apart then start 17 rows apart, in different banks, which matters when
// several groups share a wavefront (TW < 64).
template <int TW, int NQ>
__global__ __launch_bounds__(DIAG_THREADS, 2) void k_diag_acov(const double* __restrict__ samples, long long n, long long S, int P, int H, int T,
                                                           int lds_rows, double* __restrict__ blk, double* __restrict__ means) {
  extern __shared__ __attribute__((aligned(16))) double dg_lds[];
  constexpr int G = DIAG_THREADS / TW;
  static_assert(DIAG_R == 16 && DIAG_THREADS % TW == 0, "the lag loop is written for 16 lags per thread");
  const int tid = threadIdx.x, dl = tid % TW, g = tid / TW;
  const long long dcol = (long long)blockIdx.x * TW + dl;
  const bool dvalid = dcol < P;
  double* tile = dg_lds;
  double* red = tile + (size_t)lds_rows * TW;
  int* bad = (int*)(red + DIAG_THREADS);
  const int tg0 = g * DIAG_R;  // lag set q of this thread starts at tg0 + q G 16
  for (int i = tid; i < lds_rows * TW; i += DIAG_THREADS) tile[i] = 0.0;
  double acc[NQ][DIAG_R];
#pragma unroll
  for (int q = 0; q < NQ; ++q)
#pragma unroll
    for (int r = 0; r < DIAG_R; ++r) acc[q][r] = 0.0;
  double used_count = 0.0, mean_sum = 0.0;
  const long long c0 = (long long)blockIdx.y * DIAG_CHAINS;
  const long long c1 = c0 + DIAG_CHAINS < n ? c0 + DIAG_CHAINS : n;
  for (long long c = c0; c < c1; ++c) {
    for (int h = 0; h < 2; ++h) {
      const double* __restrict__ x = samples + ((size_t)c * S + (size_t)(h ? S - H : 0)) * P + dcol;
      __syncthreads();  // the tile and the scratch of the previous series are no longer read
      double s = 0.0;
      int nonfinite = 0;
      if (dvalid) {
#pragma unroll 8
        for (int r = g; r < H; r += G) {
          const double v = x[(size_t)r * P];
          tile[(r + (r >> 4)) * TW + dl] = v;
          s += v;
          nonfinite |= !sum_finite(v);
        }
      }
      red[tid] = s;
      bad[tid] = nonfinite;
      __syncthreads();
      double tot = 0.0;
      int anybad = 0;
      for (int k = 0; k < G; ++k) {
        tot += red[k * TW + dl];
        anybad |= bad[k * TW + dl];
      }
      const double mu = tot / (double)H;
      const bool used = dvalid && !anybad && sum_finite(mu);
      if (dvalid)
        for (int r = g; r < H; r += G) {
          const int i = (r + (r >> 4)) * TW + dl;
          tile[i] = used ? tile[i] - mu : 0.0;
        }
      if (used) {
        used_count += 1.0;
        mean_sum += mu;
      }
      if (g == 0 && dvalid) means[(size_t)(2 * c + h) * P + dcol] = used ? mu : NAN;
      __syncthreads();
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int tg = tg0 + q * G * DIAG_R;
        if (tg >= T) continue;
        const int lim = H - tg;
        for (int s0 = 0; s0 < lim; s0 += 16) {
          const double* ap = tile + (s0 + (s0 >> 4)) * TW + dl;
          const int b = s0 + tg;
          const double* wp = tile + (b + (b >> 4)) * TW + dl;
          double w[2 * DIAG_R - 1];
#pragma unroll
          for (int j = 0; j < 2 * DIAG_R - 1; ++j) w[j] = wp[(j + (j >> 4)) * TW];
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const double a = ap[i * TW];
#pragma unroll
            for (int r = 0; r < DIAG_R; ++r) acc[q][r] = fma(a, w[i + r], acc[q][r]);
          }
        }
      }
    }
  }
  if (!dvalid) return;
  const size_t bb = (size_t)blockIdx.y * (size_t)(2 + T) * P;
  if (g == 0) {
    blk[bb + dcol] = used_count;
    blk[bb + P + dcol] = mean_sum;
  }
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int tg = tg0 + q * G * DIAG_R;
#pragma unroll
    for (int r = 0; r < DIAG_R; ++r)
      if (tg + r < T) blk[bb + (size_t)(2 + tg + r) * P + dcol] = acc[q][r];
  }
}

// blk [nblocks][2 + T][P] -> rows 0, 1, 3 and 4.. of the partial, one thread per (row, dimension), the blocks added in block order.
__global__ __launch_bounds__(256) void k_diag_reduce(const double* __restrict__ blk, long long nblocks, int P, int H, int T,
                                                     double* __restrict__ partial) {
  const size_t rowlen = (size_t)(2 + T) * P;
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= rowlen) return;
  const size_t row = i / P, d = i % P;
  double sum = 0.0;
#pragma unroll 8
  for (long long b = 0; b < nblocks; ++b) sum += blk[(size_t)b * rowlen + i];
  if (row == 0) {
    partial[d] = sum;
  } else if (row == 1) {
    double m = 0.0;
#pragma unroll 8
    for (long long b = 0; b < nblocks; ++b) m += blk[(size_t)b * rowlen + d];
    partial[P + d] = m > 0.0 ? sum / m : 0.0;
  } else {
    const double v = sum / (double)H;
    partial[(size_t)(2 + row) * P + d] = v;
    if (row == 2) partial[(size_t)3 * P + d] = v * (double)H / (double)(H - 1);
  }
}

// Row 2 of the partial, the second pass about its row 1: M2 = sum over the used series of (mean_j - row 1)^2.  A workgroup of 1024 takes
// 16 dimensions; thread (dl, g) adds the series g, g + 64, ... in that order, and the 64 sums of a dimension meet in a fixed tree.
__global__ __launch_bounds__(1024) void k_diag_m2(const double* __restrict__ means, long long nseries, int P, double* __restrict__ partial) {
  __shared__ double red[1024];
  const int tid = threadIdx.x, dl = tid & 15, g = tid >> 4;
  const long long d = (long long)blockIdx.x * 16 + dl;
  double s = 0.0;
  if (d < P) {
    const double mu = partial[P + d];
    for (long long j = g; j < nseries; j += 64) {
      const double v = means[(size_t)j * P + d];
      const double e = v - mu;
      s += (v == v) ? e * e : 0.0;
    }
  }
  red[tid] = s;
  __syncthreads();
  for (int o = 32; o >= 1; o >>= 1) {
    if (g < o) red[tid] += red[tid + o * 16];
    __syncthreads();
  }
  if (g == 0 && d < P) partial[(size_t)2 * P + d] = red[tid];
}
