// Posterior predictive probabilities of rows xnew [R][D] under the draws w [N][D] in device memory (include/rmhmc_pred.h): the partial of
// pred.h.  N = n S rows of a *_sample_to buffer [n][S][D], D <= PRED_MAX_D.  An R x N x D product on v_mfma_f64_16x16x4_f64 with a sigmoid
// epilogue and a reduction over the draws.
//
// Three kernels, no atomics; every sum has a fixed order that depends on (N, R, D) alone, so a call repeats bit for bit.
//   k_pred_valid  grid: the draw blocks of the validity pass (pred_plan) x 256 threads.  A wavefront takes the draws wv, wv + 4, ... of
//                 its block, lane l the columns l, l + 64, ...: a draw with a non-finite entry (wave_row_finite) gets valid[] = 0,
//                 the others 1.  The four wavefronts' counts meet in LDS: cnt [blocks], the draws used in each.
//   k_pred_main   grid: (row tiles of PRED_ROW_TILE rows, draw blocks) x PRED_WAVES wavefronts.  A wavefront owns 16 rows of xnew as the A
//                 operand, lane l holding A[i = l & 15][k = l >> 4] = xnew[row0 + i][4 s + k] of every step s in registers (KS doubles:
//                 the kernel is compiled for KS = 4, 8, 16, .., 64 steps, pred_ksteps: ceil(D / 4) rounded up), and walks the draws of its
//                 block 16 at a time: B[k][j = l & 15] = w[j0 + j][4 s + k] read straight from global memory (a quarter wavefront reads 32
//                 consecutive bytes of each of 16 draws; the four wavefronts of a workgroup read the same draws and share them through the
//                 L1), with no branch in the product, so that the loads of a tile are in flight together.  Exact zeros for k >= D and
//                 rows >= R (in A), draws past the end and flagged draws (in B): padding never shows in the product.  A padded or
//                 flagged draw is also kept out of the sums (f = 0 would add p = 1/2): its lanes skip the epilogue.  Result
//                 element e of lane l is f of row (l >> 4) + 4 e and draw l & 15: the epilogue takes the sigmoid of include/rmhmc_pred.h on
//                 each and adds p, p^2 and q to the lane's sum_pairs (sums.hip.h) of its four rows, across the whole block.
//                 At the end the 16 draw lanes of a row are added by a butterfly (xor 8, 4, 2, 1) and lane 0 of each quarter rounds sum +
//                 error into the record rec [row tile][block][3][PRED_ROW_TILE].
//   k_pred_fin    one thread per row: the records added in block order (pairs again), the counts added (exact integers), the four rows
//                 of the partial written; without labels row 3 is -0.0.
// The epilogue (an exp, a division, three two-sums per f), not the product, is the larger cost: the xnew tile stays in registers and the
// draws are read once per row tile.  Neither goes through LDS.
#pragma once
#include <hip/hip_runtime.h>

#include "pred.h"      // PRED_MAX_D, the row tile, the blocks
#include "sums.hip.h"  // sum_pair, block_rows, wave_row_finite, d4

static_assert(PRED_MAX_D == 256, "wave_row_finite checks 256 columns");

__global__ __launch_bounds__(256) void k_pred_valid(const double* __restrict__ w, size_t N, int D, size_t draws_per_block,
                                                    unsigned char* __restrict__ valid, double* __restrict__ cnt) {
  __shared__ double red_m[4];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const block_range draws = block_rows(blockIdx.x, draws_per_block, N);
  double used = 0.0;
  for (size_t j = draws.begin + wv; j < draws.end; j += 4) {
    double v[4];
    const bool ok = wave_row_finite(w + j * (size_t)D, D, lane, v);
    if (lane == 0) valid[j] = ok ? 1 : 0;
    if (ok) used += 1.0;
  }
  if (lane == 0) red_m[wv] = used;
  __syncthreads();
  if (tid == 0) cnt[blockIdx.x] = ((red_m[0] + red_m[1]) + red_m[2]) + red_m[3];
}

// The rows-by-draws product of a wavefront: 16 rows of x [nrows][D] from row0 on as the A operand, KS steps of four columns, against 16
// draws at a time.  Lane l holds A[i = l & 15][k = l >> 4]; result element e of lane l is row (l >> 4) + 4 e and draw l & 15.
template <int KS>
struct DrawProduct {
  // the last TAIL steps may reach past column D: their A is zero there and their B comes from a clamped column, a finite number
  // (the draw is valid or its lanes select zero), so the product is an exact zero; the steps before them are all inside
  static constexpr int TAIL = KS < 8 ? KS : 8;
  double xa[KS];
  unsigned toff[TAIL];
  bool one[4];  // the label of the row of result element e is 1
  int k;

  // t: the labels [nrows], or nullptr for none
  __device__ __forceinline__ void load(const double* __restrict__ x, const double* __restrict__ t, size_t row0, size_t nrows, int D, int lane) {
    k = lane >> 4;
    const size_t ra = row0 + (size_t)(lane & 15);
    const size_t rc = ra < nrows ? ra : nrows - 1;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int c = 4 * s + k;
      const double v = x[rc * (size_t)D + (size_t)(c < D ? c : D - 1)];
      xa[s] = (ra < nrows && c < D) ? v : 0.0;
    }
#pragma unroll
    for (int u = 0; u < TAIL; ++u) {
      const int c = 4 * (KS - TAIL + u) + k;
      toff[u] = (unsigned)(c < D ? c : D - 1);
    }
#pragma unroll
    for (int el = 0; el < 4; ++el) {
      const size_t rr = row0 + (size_t)(k + 4 * el);
      one[el] = t != nullptr && rr < nrows && t[rr] == 1.0;
    }
  }

  // f of the 16 rows under the lane's draw j of the block's [.., j_end); ok: the draw exists and is not flagged (else its f is zero).
  // Branch-free, so that the loads of a tile are in flight together: a lane without a draw reads draw j_end - 1, which exists, and
  // selects zero.
  __device__ __forceinline__ d4 times(const double* __restrict__ w, const unsigned char* __restrict__ valid, int D, size_t j, size_t j_end,
                                      bool& ok) const {
    const size_t jc = j < j_end ? j : j_end - 1;
    ok = j < j_end && valid[jc] != 0;
    const double* __restrict__ wr = w + jc * (size_t)D;
    d4 acc = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < KS - TAIL; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[s], ok ? wr[4 * s + k] : 0.0, acc, 0, 0, 0);
#pragma unroll
    for (int u = 0; u < TAIL; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[KS - TAIL + u], ok ? wr[toff[u]] : 0.0, acc, 0, 0, 0);
    return acc;
  }
};

template <int KS>
__global__ __launch_bounds__(64 * PRED_WAVES) void k_pred_main(const double* __restrict__ w, size_t N, int D, size_t draws_per_block,
                                                               const unsigned char* __restrict__ valid, const double* __restrict__ xnew,
                                                               const double* __restrict__ tnew /* nullptr: no labels */, size_t R,
                                                               double* __restrict__ rec) {
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, a = lane & 15, k = lane >> 4;
  const size_t row0 = (size_t)blockIdx.x * PRED_ROW_TILE + (size_t)wv * PRED_WAVE_ROWS;
  if (row0 >= R) return;  // (the whole wavefront: its rows of the record are never read)
  DrawProduct<KS> xw;
  xw.load(xnew, tnew, row0, R, D, lane);
  sum_pair s1[4] = {}, s2[4] = {}, sq[4] = {};
  const block_range draws = block_rows(blockIdx.y, draws_per_block, N);  // (begin a multiple of 16)
  for (size_t j0 = draws.begin; j0 < draws.end; j0 += 16) {
    bool ok;
    const d4 acc = xw.times(w, valid, D, j0 + (size_t)a, draws.end, ok);
    if (ok) {
#pragma unroll
      for (int el = 0; el < 4; ++el) {
        const double f = acc[el];
        const double ex = exp(-fabs(f));
        const double den = 1.0 + ex;
        const double hi = 1.0 / den, lo = ex / den;
        const bool pos = f >= 0.0;
        const double p = pos ? hi : lo, np = pos ? lo : hi;
        s1[el].add(p);
        s2[el].add(p * p);
        sq[el].add(xw.one[el] ? p : np);
      }
    }
  }
  // the 16 draw lanes of a row, in a fixed order; the result is read from lane a = 0
  auto partner = [](const sum_pair& v, int mask) { return sum_pair{__shfl_xor(v.s, mask, 64), __shfl_xor(v.e, mask, 64)}; };
#pragma unroll
  for (int el = 0; el < 4; ++el) {
#pragma unroll
    for (int mask = 8; mask >= 1; mask >>= 1) {
      const sum_pair o1 = partner(s1[el], mask), o2 = partner(s2[el], mask), oq = partner(sq[el], mask);
      s1[el].add(o1);
      s2[el].add(o2);
      sq[el].add(oq);
    }
  }
  if (a == 0) {
    double* out = rec + ((size_t)blockIdx.x * gridDim.y + blockIdx.y) * 3 * PRED_ROW_TILE + (size_t)wv * PRED_WAVE_ROWS;
#pragma unroll
    for (int el = 0; el < 4; ++el) {
      const int i = k + 4 * el;
      out[i] = s1[el].value();
      out[PRED_ROW_TILE + i] = s2[el].value();
      out[2 * PRED_ROW_TILE + i] = sq[el].value();
    }
  }
}

// rec [row tiles][nblocks][3][PRED_ROW_TILE], cnt [vblocks] -> the partial [4][R]
__global__ __launch_bounds__(256) void k_pred_fin(const double* __restrict__ rec, size_t nblocks, const double* __restrict__ cnt,
                                                  size_t vblocks, size_t R, int has_labels, double* __restrict__ partial) {
  const size_t r = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  double m = 0.0;
  for (size_t b = 0; b < vblocks; ++b) m += cnt[b];
  const double* in = rec + (r / PRED_ROW_TILE) * nblocks * 3 * PRED_ROW_TILE + r % PRED_ROW_TILE;
  sum_pair s[3] = {};
  for (size_t b = 0; b < nblocks; ++b)
#pragma unroll
    for (int q = 0; q < 3; ++q) s[q].add(in[(b * 3 + (size_t)q) * PRED_ROW_TILE]);
  partial[r] = m;
  partial[R + r] = s[0].value();
  partial[2 * R + r] = s[1].value();
  partial[3 * R + r] = has_labels ? s[2].value() : -0.0;
}
