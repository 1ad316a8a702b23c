// Leave-one-out cross-validation (include/rmhmc_loo.h): the log-likelihood matrix ll [N][C] of C <= LOO_MAX_COLS data rows under the draws
// w [N][D] in device memory, its moments, the split at the cutoff and the generalised Pareto fit of every column's tail.  The cutoff
// itself is the select of quant.hip.h on ll.  Every floating-point sum has a fixed order that depends on N alone (not on C, so a column
// gives the same bits whichever block of columns it is computed in); the one atomic is the integer slot counter of the gather.
//
//   k_loo_loglik   grid: blocks of LOO_DRAWS draws x 4 wavefronts.  A wavefront owns 16 columns (data rows) as the A operand of the
//                  DrawProduct of pred.hip.h and walks the draws of the block 16 at a time: exact zeros for k >= D and columns >= C (in
//                  A) and for draws past the end or flagged by k_pred_valid (in B).  The MFMA steps of an (x, w) pair are the same whichever
//                  lane holds them, so l does not depend on the position of the draw or the column.  Epilogue: l of include/rmhmc_loo.h;
//                  result element e of lane l is column (l >> 4) + 4 e and draw l & 15; a flagged draw writes NaN, a draw past the end
//                  nothing.
//   k_loo_reduce   grid: the row blocks of loo_kernel_plan x 256 threads = LOO_ROW_LANES row lanes (one wavefront each) x 64 columns:
//                  thread (g, c) walks rows g, g + 4, .. of its block with the sum_pairs of sums.hip.h; the four lanes of a
//                  column meet in LDS in lane order and leave one record rec [block][LOO_REC][64].  MODE 0: count, sum l, sum exp(l),
//                  min l.  MODE 1: sum (l - mean)^2.  MODE 2: n_lt, n_gt, n_eq and sum over l > cut of exp(lmin - l); a value below the
//                  cutoff takes the next slot of its column's tail.
//   k_loo_fin<MODE> one thread per column adds the records in block order and writes the partial (MODE 0: rows 0, 1, 3, 4; MODE 1: row 2)
//                  or the counts and the body (MODE 2).
//   k_loo_fit      one workgroup per column, the tail in LDS (dynamic, LOO_FIT_LDS_BYTES): bitonic sort, the sorted l to global scratch,
//                  y in place, the G candidates of Zhang and Stephens one block reduction each, the smoothed weights and their two sums.
#pragma once
#include <hip/hip_runtime.h>

#include "loo.h"
#include "pred.hip.h"  // DrawProduct, k_pred_valid
#include "sums.hip.h"  // sum_pair, sum_finite, block_rows

#define LOO_FIT_LDS_DOUBLES (LOO_MAX_TAIL + 2 * LOO_MAX_G + 2 * LOO_FIT_THREADS + 8)
#define LOO_FIT_LDS_BYTES (LOO_FIT_LDS_DOUBLES * 8)

template <int KS>
__global__ __launch_bounds__(256) void k_loo_loglik(const double* __restrict__ w, size_t N, int D, const unsigned char* __restrict__ valid,
                                                    const double* __restrict__ x, const double* __restrict__ t, int C,
                                                    double* __restrict__ ll) {
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, a = lane & 15, k = lane >> 4;
  const int col0 = wv * 16;
  if (col0 >= C) return;  // (the whole wavefront)
  DrawProduct<KS> xw;
  xw.load(x, t, (size_t)col0, (size_t)C, D, lane);
  const block_range draws = block_rows(blockIdx.x, LOO_DRAWS, N);
  for (size_t j0 = draws.begin; j0 < draws.end; j0 += 16) {
    const size_t j = j0 + (size_t)a;
    bool ok;
    const d4 acc = xw.times(w, valid, D, j, draws.end, ok);
    if (j < draws.end) {
#pragma unroll
      for (int el = 0; el < 4; ++el) {
        const int cc = col0 + k + 4 * el;
        const double f = acc[el];
        const double s = xw.one[el] ? f : -f;
        const double ex = exp(-fabs(f));
        double l = (s < 0.0 ? s : 0.0) - log1p(ex) + 0.0;  // (+ 0.0: a -0.0 becomes +0.0)
        if (!ok || f != f) l = __builtin_nan("");
        if (cc < C) ll[j * (size_t)C + (size_t)cc] = l;
      }
    }
  }
}

// the arguments of MODE 2 (the split), all [C] in device memory but the tail [C][stride]
struct loo_split_args {
  const double* cut;
  const double* lmin;
  const long long* tail_len;
  double* tail;
  long long stride;
  unsigned long long* fill;  // the slot counters, zero before the launch
};

template <int MODE>
__global__ __launch_bounds__(256) void k_loo_reduce(const double* __restrict__ ll, size_t N, int C, size_t rows_per_block,
                                                    const double* __restrict__ mean, loo_split_args sp, double* __restrict__ rec) {
  __shared__ sum_pair red[LOO_ROW_LANES][LOO_REC][LOO_MAX_COLS];
  const int tid = threadIdx.x, c = tid & 63, g = tid >> 6;
  const bool mine = c < C;
  const block_range rows = block_rows(blockIdx.x, rows_per_block, N);
  sum_pair s[LOO_REC] = {};  // (a count or the minimum lives in .s alone)
  if (MODE == 0) s[3].s = __builtin_inf();
  double mu = 0.0, cut = 0.0, lmin = 0.0;
  long long tl = 0;
  if (mine && MODE == 1) mu = mean[c];
  if (mine && MODE == 2) { cut = sp.cut[c]; lmin = sp.lmin[c]; tl = sp.tail_len[c]; }
  const bool smoothed = tl >= 5;
  if (mine) {
    for (size_t r = rows.begin + (size_t)g; r < rows.end; r += LOO_ROW_LANES) {
      const double l = ll[r * (size_t)C + (size_t)c];
      if (!sum_finite(l)) continue;
      if (MODE == 0) {
        s[0].s += 1.0;
        s[1].add(l);
        s[2].add(exp(l));
        s[3].s = l < s[3].s ? l : s[3].s;
      } else if (MODE == 1) {
        const double dl = l - mu;
        s[0].add(dl * dl);
      } else {
        if (smoothed && l < cut) {
          s[0].s += 1.0;
          const unsigned long long slot = atomicAdd(&sp.fill[c], 1ull);
          if (slot < (unsigned long long)tl) sp.tail[(size_t)c * (size_t)sp.stride + (size_t)slot] = l;  // (tl <= stride: checked on the host)
        } else if (smoothed && !(l > cut)) {
          s[2].s += 1.0;
        } else {
          s[1].s += 1.0;
          s[3].add(exp(lmin - l));
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < LOO_REC; ++q) red[g][q][c] = s[q];
  __syncthreads();
  if (g == 0 && mine) {
    double* out = rec + (size_t)blockIdx.x * LOO_REC * LOO_MAX_COLS + c;
#pragma unroll
    for (int q = 0; q < LOO_REC; ++q) {
      sum_pair t = red[0][q][c];
      for (int l = 1; l < LOO_ROW_LANES; ++l) {
        if (MODE == 0 && q == 3) { t.s = red[l][q][c].s < t.s ? red[l][q][c].s : t.s; continue; }
        t.add(red[l][q][c]);
      }
      out[q * LOO_MAX_COLS] = t.value();
    }
  }
}

// MODE 0: rec -> partial rows 0 (m), 1 (mean), 3 (SQ), 4 (lmin); MODE 1: rec -> partial row 2 (M2); MODE 2: rec -> counts [2][C], body [2][C]
template <int MODE>
__global__ __launch_bounds__(64) void k_loo_fin(const double* __restrict__ rec, size_t nblocks, int C, double* __restrict__ partial,
                                                loo_split_args sp, long long* __restrict__ counts, double* __restrict__ body) {
  const int c = threadIdx.x;
  if (c >= C) return;
  sum_pair s[LOO_REC] = {};
  if (MODE == 0) s[3].s = __builtin_inf();
  for (size_t b = 0; b < nblocks; ++b) {
    const double* in = rec + b * LOO_REC * LOO_MAX_COLS + c;
#pragma unroll
    for (int q = 0; q < LOO_REC; ++q) {
      const double v = in[q * LOO_MAX_COLS];
      if (MODE == 0 && q == 3) s[3].s = v < s[3].s ? v : s[3].s;
      else s[q].add(v);
    }
  }
  const size_t n = (size_t)C;
  if (MODE == 0) {
    const double m = s[0].s;
    partial[c] = m;
    partial[n + c] = m > 0.0 ? s[1].value() / m : 0.0;
    partial[3 * n + c] = s[2].value();
    partial[4 * n + c] = s[3].s;
  } else if (MODE == 1) {
    partial[2 * n + c] = s[0].value();
  } else {
    const double n_lt = s[0].s, n_gt = s[1].s, n_eq = s[2].s;
    const double lmin = sp.lmin[c];
    double A = 0.0, B = 0.0;
    if (n_lt + n_gt + n_eq > 0.0) {
      double rest = n_eq;  // the copies of the cutoff that stay in the body: n_eq - r, r = M - n_lt
      if (sp.tail_len[c] >= 5) rest = n_eq - ((double)sp.tail_len[c] - n_lt);
      if (rest > 0.0) s[3].add(rest * exp(lmin - sp.cut[c]));
      A = s[3].value();
      B = (n_gt + rest) * exp(lmin);
    }
    counts[c] = (long long)n_lt;
    counts[n + c] = (long long)n_gt;
    body[c] = A;
    body[n + c] = B;
  }
}

// the sum of the threads' pairs in a fixed tree; every thread of the workgroup calls it and gets the sum
__device__ __forceinline__ double loo_block_sum(sum_pair v, sum_pair* red, int tid) {
  __syncthreads();  // (whoever still reads the last sum is done)
  red[tid] = v;
  __syncthreads();
  for (int h = LOO_FIT_THREADS / 2; h >= 1; h >>= 1) {
    if (tid < h) {
      sum_pair a = red[tid];
      a.add(red[tid + h]);
      red[tid] = a;
    }
    __syncthreads();
  }
  return red[0].value();
}

// tail [C][stride], counts [2][C], cut, lmin, tail_len [C], sorted [C][stride] (scratch) -> fit [4][C]
__global__ __launch_bounds__(LOO_FIT_THREADS) void k_loo_fit(const double* __restrict__ tail, const long long* __restrict__ counts,
                                                             const double* __restrict__ cutv, const double* __restrict__ lminv,
                                                             const long long* __restrict__ tail_len, long long stride, int C,
                                                             double* __restrict__ sorted, double* __restrict__ fit) {
  extern __shared__ __attribute__((aligned(16))) double loo_lds[];
  double* y = loo_lds;                          // the tail: l, then y, by ascending l
  double* theta = loo_lds + LOO_MAX_TAIL;       // [LOO_MAX_G]
  double* Lv = theta + LOO_MAX_G;               // [LOO_MAX_G]
  sum_pair* red = (sum_pair*)(Lv + LOO_MAX_G);  // [LOO_FIT_THREADS]
  double* scal = Lv + LOO_MAX_G + 2 * LOO_FIT_THREADS;  // [8]
  const int tid = threadIdx.x, c = blockIdx.x;
  const size_t n = (size_t)C;
  long long Ml = tail_len[c];
  Ml = Ml > LOO_MAX_TAIL ? LOO_MAX_TAIL : Ml > stride ? stride : Ml;  // (refused on the host; the bound of the LDS and of a row)
  const int M = (int)Ml;
  if (M < 5) {
    if (tid == 0) { fit[c] = __builtin_inf(); fit[n + c] = __builtin_nan(""); fit[2 * n + c] = 0.0; fit[3 * n + c] = 0.0; }
    return;
  }
  const double cut = cutv[c], lmin = lminv[c];
  long long nl = counts[c];
  nl = nl < 0 ? 0 : nl > Ml ? Ml : nl;
  const int n_lt = (int)nl;
  int P2 = 8;
  while (P2 < M) P2 *= 2;
  const double* trow = tail + (size_t)c * (size_t)stride;
  double* srow = sorted + (size_t)c * (size_t)stride;
  for (int i = tid; i < P2; i += LOO_FIT_THREADS) y[i] = i < n_lt ? trow[i] : i < M ? cut : __builtin_inf();
  __syncthreads();
  for (int k = 2; k <= P2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P2; i += LOO_FIT_THREADS) {
        const int o = i ^ j;
        if (o > i) {
          const double a = y[i], b = y[o];
          if ((a > b) == ((i & k) == 0)) { y[i] = b; y[o] = a; }
        }
      }
      __syncthreads();
    }
  // rank j = 1 .. M of ascending lw is index M - j of ascending l
  for (int i = tid; i < M; i += LOO_FIT_THREADS) {
    const double l = y[i];
    srow[i] = l;
    y[i] = expm1(cut - l);
  }
  __syncthreads();
  const int q = (M + 2) / 4;  // floor(M / 4 + 0.5)
  const double yM = y[0], yq = y[M - q];
  bool smooth = yM > 0.0 && yq > 0.0;
  double khat = __builtin_inf(), sigma = __builtin_nan("");
  if (smooth) {
    int G = 30;
    while ((long long)(G - 30 + 1) * (G - 30 + 1) <= (long long)M) ++G;  // 30 + floor(sqrt(M))
    for (int i = 1; i <= G; ++i) {
      const double th = 1.0 / yM + (1.0 - sqrt((double)G / ((double)i - 0.5))) / (3.0 * yq);
      sum_pair s = {};
      for (int j = tid; j < M; j += LOO_FIT_THREADS) s.add(log1p(-th * y[j]));
      const double kappa = loo_block_sum(s, red, tid) / (double)M;
      if (tid == 0) {
        theta[i - 1] = th;
        Lv[i - 1] = (double)M * (log(-th / kappa) - kappa - 1.0);
      }
    }
    __syncthreads();
    if (tid == 0) {
      double mx = Lv[0];
      for (int i = 1; i < G; ++i) mx = Lv[i] > mx ? Lv[i] : mx;
      double den = 0.0, num = 0.0;
      for (int i = 0; i < G; ++i) {
        const double wgt = exp(Lv[i] - mx);  // (a NaN candidate makes the fit NaN: no smoothing)
        den += wgt;
        num += wgt * theta[i];
      }
      scal[0] = num / den;
    }
    __syncthreads();
    const double th = scal[0];
    sum_pair s = {};
    for (int j = tid; j < M; j += LOO_FIT_THREADS) s.add(log1p(-th * y[j]));
    const double kk = loo_block_sum(s, red, tid) / (double)M;
    sigma = -kk / th;
    khat = (kk * (double)M + 5.0) / ((double)M + 10.0);
    if (!sum_finite(khat) || !sum_finite(sigma)) {
      smooth = false;
      khat = __builtin_inf();
    }
  }
  const double lw_cut = lmin - cut;
  sum_pair sa = {}, sb = {};
  for (int j = 1 + tid; j <= M; j += LOO_FIT_THREADS) {
    const double l = srow[M - j];
    double lw = lmin - l;
    if (smooth) {
      const double lp = log1p(-((double)j - 0.5) / (double)M);
      const double qj = khat == 0.0 ? -sigma * lp : sigma * expm1(-khat * lp) / khat;
      lw = lw_cut + log1p(qj);
      lw = lw < 0.0 ? lw : 0.0;
    }
    sa.add(exp(lw));
    sb.add(exp(lw + l));
  }
  const double A = loo_block_sum(sa, red, tid);
  const double B = loo_block_sum(sb, red, tid);
  if (tid == 0) { fit[c] = khat; fit[n + c] = sigma; fit[2 * n + c] = A; fit[3 * n + c] = B; }
}
