// gibbs.hip.h — the reference's auxiliary-variable Gibbs sampler (Holmes and Held; code/gibbs_sampler.py:14-139) on gfx950, on the
// helpers of kernels.hip.h.  D <= 64, fp64 throughout (the int8 metric flags of the context do not apply: the row weights
// 1/lam are not the p(1-p) the slicing was certified for, so the weighted Gram matrix always goes through k_assemble on the fp64 matrix
// cores, one row range per chain whatever the batch, so that a chain's sums do not depend on the batch it runs in).
//
// State per chain: Z [Mp] (latent), lam [Mp] (mixing weights, start 1), ilam [Mp] = 1/lam for rows < M and 0 for the padding rows
// (the row-weight vector of k_assemble), B, beta [DP].  One iteration is six launches:
//   k_assemble<NB>      G = X' diag(1/lam) X + I/v                                                  (gibbs_sampler.py:102)
//   k_gibbs_factor<NB>  V = G^-1 (chol_lds_blk + spd_inverse_lds), then L = chol(V) in the same packed LDS image      (:102-103)
//   k_gibbs_b           B = V X'(Z/lam): one pass over X per chain, four wavefronts on interleaved rows, then the mat-vec   (:104-105)
//   k_gibbs_sweep<NB>   the row sweep (:109-126), one wavefront per chain, blocks of 16 consecutive rows (the draw of a row is evaluated
//                       wave-uniformly from that row's broadcast scalars): S_b = V X_b' and
//                       P_b = X_b S_b on the fp64 matrix cores, m0 = X_b B; row i of the block then needs only
//                       m_i = m0_i + sum_{k<i} delta_k P_b[i][k], delta_k = (Z_k - z_old_k)/lam_k - one broadcast and one FMA per
//                       finished row - and the block ends with B += S_b delta.  V stays in LDS for the whole sweep.
//   k_gibbs_beta        beta = B + L T, sample write-out                                            (:128-131)
//   k_gibbs_mix         r_j = |Z_j - x_j.beta| and the rejection sampler of the mixing weights, thread = row           (:50-70,133-135)
//
// Truncated normal (gibbs_truncnorm): x = m + s Phi^-1(p), p = U Phi(-m/s), on (-inf, 0) (for p > 1/2 as -Phi^-1(1 - p), 1 - p summed
// without cancellation), its mirror image on (0, inf); for m/s > 25, where
// Phi(-m/s) heads for underflow, the same quantile from the asymptotic series of log Phi (no cancellation, result -s delta, delta > 0).
// The result is finite and strictly on the label's side of 0 for every finite m, s > 0 and U in (0, 1).
//
// Bounds of the mixing-weight sampler: GIBBS_MAX_ATTEMPTS attempts per row and GIBBS_MAX_TERMS series terms per test (the reference
// loops without bound; measured on it: 2.1 attempts on average, 24 at most, series depth <= 4; an attempt succeeds about every second
// time).  A series that runs into its bound counts as a rejection; a row that runs into either bound keeps its last proposal and
// adds one to the chain's capped counter.  A NaN residual runs into the bounds.
// Where the reference stops: its proposal Y = 1 + (Y - sqrt(Y (4 r + Y))) / (2 r) cancels twice for a small residual r and, for r below
// about 1e-7, can round to exactly 0 (lam_j = r / Y = inf, accepted by the right series) or below 0 (lam_j < 0: the reference's left
// series then loops for ever on log of a negative number; here it reaches its bound and the attempt counts as rejected).  With lam_j =
// inf the reference's next sweep ends in SciPy's ValueError (scale must be positive).  Here a chain whose draw of lam_j is not a positive
// finite number stops (GibbsParams::stop = 2): every later kernel skips it, its later samples stay NaN, the iteration is reported.
//
// Random streams: Philox4x32-10 (kernels.hip.h), key = seed, counter = (chain, row, iteration, block), chain = chain_offset + c < 2^32:
//   block 0x60000000, iteration 0, row j        U0 -> the uniform of the initial Z_j
//   block 0x61000000, iteration i, row j        U0 -> the uniform of the sweep's draw of Z_j
//   block 0x62000000 + d/2, iteration i, row 0  Box-Muller pair -> T_d (cos for even d, sin for odd)
//   block 0x63000000 + 2a, iteration i, row j   Box-Muller (cos) -> the normal of attempt a; block + 1: U0, U1 -> its two uniforms
// Nothing depends on how a run is cut into launches.  The replay entry point reads all of these from tapes instead.
#pragma once
#include "kernels.hip.h"

#define GIBBS_MAX_ATTEMPTS 64
#define GIBBS_MAX_TERMS 64       // pairs of series terms
#define GIBBS_TAIL 25.0          // m/s beyond which the asymptotic tail form is used
#define GIBBS_MIX_ROWS 256

struct GibbsParams {
  unsigned long long seed;
  long long chain_offset;
  long long it;             // iteration i
  long long burn_in, S;     // samples [n][S][D]: row k = beta of iteration burn_in + k
  double* samples;          // or nullptr
  double *Z, *lam, *ilam;   // [n][Mp]
  double *B, *beta;         // [n][DP]
  double *G, *V, *Lt;       // [n][DP][DP]: G (k_assemble), V = G^-1 (full, symmetric), Lt = chol(V)' (upper)
  long long* capped;        // [n]
  int* stop;                // [n] 0: running; 1 (replay): the tape ran out of attempts for some row; 2: a draw of lam_j was not a positive
                            // finite number.  A stopped chain is skipped by every kernel from then on.
  long long* dead;          // [n] the iteration of stop = 2, or -1
  // replay (u_init != nullptr): tapes and records
  long long T;              // iterations of the tapes
  const double *u_init;     // [n][M]
  const double *u_sweep;    // [n][T][M]
  const double *T_in;       // [n][T][D]
  const double *ks;         // [n][ks_total][3]: normal, uniform, uniform of every attempt
  const long long* ks_off;  // [n][T][M+1]
  long long ks_total;
  double *beta_out, *B_out; // [n][T][D]
  int* att_out;             // [n][T][M]
};

__device__ __forceinline__ void gibbs_rng(const GibbsParams& p, int c, uint32_t row, uint32_t iter, uint32_t block, double& U0, double& U1) {
  uint32_t k[4] = {(uint32_t)(p.chain_offset + c), row, iter, block};
  philox4x32_10(k, (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
  U0 = u53(k[0], k[1]);
  U1 = u53(k[2], k[3]);
}

__device__ __forceinline__ double gibbs_Phi(double x) { return 0.5 * erfc(-0.70710678118654752440 * x); }

// Phi^-1(p), 0 < p <= 1/2 (the caller mirrors the upper half): the library's quantile, polished by one Newton step on Phi where
// Phi(y) - p keeps its relative accuracy (y < 0)
__device__ __forceinline__ double gibbs_ndtri(double p) {
  double y = normcdfinv(p);
  if (y < 0.0) {
    const double pdf = 0.39894228040143267794 * exp(-0.5 * y * y);
    if (pdf > 0.0) y -= (gibbs_Phi(y) - p) / pdf;
  }
  return y;
}

// R(y) = 1 - 1/y^2 + 3/y^4 - 15/y^6 + ... (8 terms; y^2 >= 625: the first omitted term is below 1e-17): Phi(y) = phi(y) R(y) / (-y), y < 0
__device__ __forceinline__ double gibbs_mills(double y) {
  const double q = 1.0 / (y * y);
  double r = 1.0;
#pragma unroll
  for (int k = 8; k >= 1; --k) r = 1.0 - (2 * k - 1) * q * r;
  return r;
}

// N(m, s^2) truncated to (-inf, 0) at the uniform U; Uc = 1 - U, given apart so that the mirrored call keeps the digits of a tiny uniform.
// Not inlined: inside the sweep's row loop the compiler otherwise hoists the ~250 polynomial
// constants of erfc / normcdfinv out of the loop into registers (256 VGPRs + 256 AGPRs and scratch; 92-134 VGPRs and no scratch this way).
__device__ __noinline__ double gibbs_truncnorm_neg(double U, double Uc, double m, double s) {
  const double a = m / s;
  double x;
  if (a > GIBBS_TAIL) {
    // y = Phi^-1(U Phi(-a)) = -(a + delta): log Phi(-a - delta) - log Phi(-a) = log U, Newton on delta from the exponential tail's value
    const double lu = U > 0.5 ? log1p(-Uc) : log(U), lr0 = log(gibbs_mills(a));
    double dl = -lu / a;
#pragma unroll 1
    for (int k = 0; k < 6; ++k) {
      const double y = a + dl, r = gibbs_mills(y);
      const double g = -(a + 0.5 * dl) * dl - log1p(dl / a) + (log(r) - lr0) - lu;
      dl += g * r / y;  // g' = -y / R(y)
    }
    x = -s * dl;
  } else {
    // (upper half: the quantile of the complement 1 - p = (1 - U) + U Phi(a), a sum of positive terms, keeps the digits p loses near 1)
    const double p = U * gibbs_Phi(-a);
    const double y = p > 0.5 ? -gibbs_ndtri(Uc + U * gibbs_Phi(a)) : gibbs_ndtri(fmax(p, 2.2250738585072014e-308));
    x = fma(s, y, m);
  }
  return fmin(x, -2.2250738585072014e-308);  // (rounding may land on 0 when U is within an ulp of 1)
}

// label 1: (0, inf), label 0: (-inf, 0); x = m + s * (pos ? -Phi^-1((1-U) Phi(m/s)) : Phi^-1(U Phi(-m/s)))
__device__ __forceinline__ double gibbs_truncnorm(double U, double m, double s, bool pos) {
  const double x = gibbs_truncnorm_neg(pos ? 1.0 - U : U, pos ? U : 1.0 - U, pos ? -m : m, s);
  return pos ? -x : x;
}

// the two alternating series tests (gibbs_sampler.py:14-47, as written); 1 accept, 0 reject, -1 bound reached
__device__ __forceinline__ int gibbs_rightmost(double U, double Lambda) {
  double Z = 1.0;
  const double X = exp(-0.5 * Lambda);
  int j = 0;
#pragma unroll 1
  for (int k = 0; k < GIBBS_MAX_TERMS; ++k) {
    j += 1;
    Z -= (double)((j + 1) * (j + 1)) * pow(X, (double)((j + 1) * (j + 1) - 1));
    if (Z > U) return 1;
    j += 1;
    Z += (double)((j + 1) * (j + 1)) * pow(X, (double)((j + 1) * (j + 1) - 1));
    if (Z < U) return 0;
  }
  return -1;
}
__device__ __forceinline__ int gibbs_leftmost(double U, double Lambda) {
  const double pi = 3.14159265358979323846, pi2 = pi * pi;
  const double H = 0.5 * log(2.0) + 2.5 * log(pi) - 2.5 * log(Lambda) - pi2 / (2.0 * Lambda) + 0.5 * Lambda;
  const double logU = log(U);
  double Z = 1.0;
  const double X = exp(-pi2 / (2.0 * Lambda));
  const double K = Lambda / pi2;
  int j = 0;
#pragma unroll 1
  for (int k = 0; k < GIBBS_MAX_TERMS; ++k) {
    j += 1;
    Z -= K * pow(X, (double)(j * j - 1));
    if (H + log(Z) > logU) return 1;   // (log of a negative Z: NaN, the comparison is false, as in the reference)
    j += 1;
    Z += (double)((j + 1) * (j + 1)) * pow(X, (double)((j + 1) * (j + 1) - 1));
    if (H + log(Z) < logU) return 0;
  }
  return -1;
}

// initial Z (gibbs_sampler.py:79-93), lam = 1, row weights 1 (0 in the padding rows)
__global__ __launch_bounds__(256) void k_gibbs_init(DevData dd, GibbsParams p) {
  const int c = blockIdx.x, row = blockIdx.y * 256 + threadIdx.x;
  if (row >= dd.Mp) return;
  const size_t o = (size_t)c * dd.Mp + row;
  double z = 0.0;
  if (row < dd.M) {
    double U, U1;
    if (p.u_init) U = p.u_init[(size_t)c * dd.M + row];
    else gibbs_rng(p, c, (uint32_t)row, 0u, 0x60000000u, U, U1);
    z = gibbs_truncnorm(U, 0.0, 1.0, dd.t[row] > 0.5);
  }
  p.Z[o] = z;
  p.lam[o] = 1.0;
  p.ilam[o] = row < dd.M ? 1.0 : 0.0;
  if (row == 0) { p.capped[c] = 0; p.stop[c] = 0; p.dead[c] = -1; }
}

// V = G^-1 and Lt = chol(V)' from the assembled G, packed LDS image as in k_factor_full / k_iwls_ljit
template <int NB>
__global__ __launch_bounds__(64) void k_gibbs_factor(int D, int DP, GibbsParams p) {
  __shared__ __attribute__((aligned(16))) double A[RM_PK_DOUBLES];
  constexpr int DPc = 16 * NB;
  const int c = blockIdx.x, lane = threadIdx.x;
  if (p.stop[c]) return;
  load_mat_lds<true>(A, p.G + (size_t)c * DP * DP, D, DP, lane);
  double rdiag;
  (void)chol_lds_blk<NB, true>(A, D, lane, rdiag);  // (not positive definite: NaN from here on)
  spd_inverse_lds<NB, true>(A, D, lane, rdiag);
  double* __restrict__ Vg = p.V + (size_t)c * DP * DP;
  for (int i = 0; i < DPc; ++i) {
    const double v = (lane <= i) ? A[rm_row<true>(i) + lane] : A[rm_row<true>(min(lane, DPc - 1)) + i];
    if (lane < DPc) Vg[i * DP + lane] = (i < D && lane < D) ? v : 0.0;
  }
  __builtin_amdgcn_wave_barrier();
  (void)chol_lds_blk<NB, true>(A, D, lane, rdiag);
  double* __restrict__ Lt = p.Lt + (size_t)c * DP * DP;
  for (int j = 0; j < DPc; ++j) {  // Lt[j][i] = L[i][j], i >= j
    const double v = (lane >= j && lane < DPc) ? A[rm_row<true>(lane) + j] : 0.0;
    if (lane < DPc) Lt[j * DP + lane] = (lane < D && j < D) ? v : 0.0;
  }
}

// B = V (X' (Z / lam)).  Wave w of the four takes the rows j = w (mod 4), two sums per wave; the partial sums are added in a fixed order.
__global__ __launch_bounds__(256) void k_gibbs_b(DevData dd, GibbsParams p) {
  __shared__ double ys[4][64];
  const int c = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (p.stop[c]) return;
  const int DP = dd.DP, M = dd.M;
  const bool in = lane < DP;
  const double* __restrict__ Zc = p.Z + (size_t)c * dd.Mp;
  const double* __restrict__ ilc = p.ilam + (size_t)c * dd.Mp;
  const double* __restrict__ xp = dd.Xr + (in ? lane : 0);
  double y0 = 0.0, y1 = 0.0;
  int j = wv;
  for (; j + 4 < M; j += 8) {
    const double a0 = Zc[j] * ilc[j], a1 = Zc[j + 4] * ilc[j + 4];
    y0 = fma(xp[(size_t)j * DP], a0, y0);
    y1 = fma(xp[(size_t)(j + 4) * DP], a1, y1);
  }
  if (j < M) y0 = fma(xp[(size_t)j * DP], Zc[j] * ilc[j], y0);
  ys[wv][lane] = in ? y0 + y1 : 0.0;
  __syncthreads();
  if (wv) return;
  const double y = (ys[0][lane] + ys[1][lane]) + (ys[2][lane] + ys[3][lane]);
  const double* __restrict__ Vg = p.V + (size_t)c * DP * DP;
  double b = 0.0;
  for (int k = 0; k < dd.D; ++k) b = fma(in ? Vg[k * DP + lane] : 0.0, rdlane(y, k), b);  // (V symmetric: row k read coalesced)
  if (in) p.B[(size_t)c * DP + lane] = b;
}

// The sweep.  Lane (kk, ii) = (lane >> 4, lane & 15); the row scalars of block row ii live on the four lanes with that ii.
template <int NB>
__global__ __launch_bounds__(64) void k_gibbs_sweep(DevData dd, GibbsParams p) {
  constexpr int DP = 16 * NB, LD = DP + 2, NK = DP / 4;
  __shared__ __attribute__((aligned(16))) double Vs[DP * LD];
  __shared__ double Bs[64], Ps[16 * 17];
  const int c = blockIdx.x, lane = threadIdx.x, ii = lane & 15, kk = lane >> 4;
  if (p.stop[c]) return;
  const int M = dd.M;
  const double* __restrict__ Vg = p.V + (size_t)c * DP * DP;
  if (lane < DP)
    for (int i = 0; i < DP; ++i) Vs[i * LD + lane] = Vg[i * DP + lane];
  Bs[lane] = lane < DP ? p.B[(size_t)c * DP + lane] : 0.0;
  __syncthreads();
  double* __restrict__ Zc = p.Z + (size_t)c * dd.Mp;
  const double* __restrict__ lamc = p.lam + (size_t)c * dd.Mp;
#pragma unroll 1
  for (int r0 = 0; r0 < M; r0 += 16) {
    const int row = r0 + ii;
    const bool live = row < M;
    // operand registers: x[q] = X[r0 + ii][4q + kk] (the padding rows and columns of Xr are zero)
    double x[NK];
    const double* __restrict__ xp = dd.Xr + (size_t)row * DP + kk;
#pragma unroll
    for (int q = 0; q < NK; ++q) x[q] = xp[4 * q];
    const double lam = live ? lamc[row] : 1.0, zold = live ? Zc[row] : 0.0;
    const bool pos = dd.t[row] > 0.5;
    double U = 0.5, U1;
    if (live) {
      if (p.u_sweep) U = p.u_sweep[((size_t)c * p.T + p.it) * M + row];
      else gibbs_rng(p, c, (uint32_t)row, (uint32_t)p.it, 0x61000000u, U, U1);
    }
    // S_b = V X_b' (tile I: rows 16I.., columns = block rows): A[i][k] = V[16I + i][4q + k], B[k][j] = X[r0 + j][4q + k]
    d4 S[NB];
#pragma unroll
    for (int I = 0; I < NB; ++I) {
      S[I] = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int q = 0; q < NK; ++q) S[I] = __builtin_amdgcn_mfma_f64_16x16x4f64(Vs[(16 * I + ii) * LD + 4 * q + kk], x[q], S[I], 0, 0, 0);
    }
    // P_b = X_b S_b: the accumulator S[I][r] holds S_b[16I + 4r + kk][ii], which is the B operand of the k chunk 16I + 4r
    d4 P = (d4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int I = 0; I < NB; ++I)
#pragma unroll
      for (int r = 0; r < 4; ++r) P = __builtin_amdgcn_mfma_f64_16x16x4f64(x[4 * I + r], S[I][r], P, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) Ps[(kk + 4 * r) * 17 + ii] = P[r];  // P[r] = P_b[kk + 4r][ii]
    // m0 = X_b B
    double m0 = 0.0;
#pragma unroll
    for (int q = 0; q < NK; ++q) m0 = fma(x[q], Bs[4 * q + kk], m0);
    m0 = col4_sum(m0);
    __syncthreads();
    const double h = Ps[ii * 17 + ii];
    const double w = h / (lam - h);
    const double sd = sqrt(lam * (w + 1.0));
    double macc = 0.0, delta = 0.0, znew = zold;
    const int nrow = min(16, M - r0);
#pragma unroll 1
    for (int k = 0; k < nrow; ++k) {
      const double pk = Ps[ii * 17 + k];
      double m = m0 + macc;
      m -= w * (zold - m);
      // row k's scalars broadcast from its lane: the draw is evaluated once, wave-uniformly (no lane takes another branch of it)
      const double zo = rdlane(zold, k);
      const bool pk1 = __builtin_amdgcn_readlane((int)pos, k) != 0;
      const double zk = gibbs_truncnorm(rdlane(U, k), rdlane(m, k), rdlane(sd, k), pk1);
      const double dk = (zk - zo) / rdlane(lam, k);
      if (ii == k) { znew = zk; delta = dk; }
      macc = fma(dk, pk, macc);
    }
    if (live && kk == 0) Zc[row] = znew;
    // B += S_b delta
#pragma unroll
    for (int I = 0; I < NB; ++I)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double s = row16_sum(S[I][r] * delta);
        if (ii == 0) Bs[16 * I + 4 * r + kk] += s;
      }
    __syncthreads();
  }
  if (lane < DP) p.B[(size_t)c * DP + lane] = Bs[lane];
}

// beta = B + L T (gibbs_sampler.py:128-131), lane = dimension
__global__ __launch_bounds__(64) void k_gibbs_beta(int D, int DP, GibbsParams p) {
  const int c = blockIdx.x, lane = threadIdx.x;
  if (p.stop[c]) return;
  const bool in = lane < D;
  double Tn = 0.0;
  if (in) {
    if (p.T_in) {
      Tn = p.T_in[((size_t)c * p.T + p.it) * D + lane];
    } else {
      double U0, U1;
      gibbs_rng(p, c, 0u, (uint32_t)p.it, 0x62000000u + (uint32_t)(lane >> 1), U0, U1);
      Tn = normal_of_pair(U0, U1, lane & 1);
    }
  }
  const double* __restrict__ Lt = p.Lt + (size_t)c * DP * DP;
  const double B = in ? p.B[(size_t)c * DP + lane] : 0.0;
  double lt = 0.0;
  for (int j = 0; j < D; ++j) lt = fma(in ? Lt[j * DP + lane] : 0.0, rdlane(Tn, j), lt);  // (L T)_i = sum_j Lt[j][i] T_j
  const double beta = B + lt;
  if (!in) return;
  p.beta[(size_t)c * DP + lane] = beta;
  if (p.samples && p.it >= p.burn_in) p.samples[((size_t)c * p.S + (size_t)(p.it - p.burn_in)) * D + lane] = beta;
  if (p.beta_out) {
    const size_t r = ((size_t)c * p.T + p.it) * D + lane;
    p.beta_out[r] = beta;
    p.B_out[r] = B;
  }
}

// mixing weights (gibbs_sampler.py:50-70,133-135): thread = row, blockIdx.x = chain
__global__ __launch_bounds__(GIBBS_MIX_ROWS) void k_gibbs_mix(DevData dd, GibbsParams p) {
  __shared__ double bs[64];
  __shared__ int stopped;  // (read once per block: other blocks of the chain may raise the flag while this one runs)
  const int c = blockIdx.x, row = blockIdx.y * GIBBS_MIX_ROWS + threadIdx.x;
  if (threadIdx.x == 0) stopped = p.stop[c];
  if (threadIdx.x < 64) bs[threadIdx.x] = threadIdx.x < dd.D ? p.beta[(size_t)c * dd.DP + threadIdx.x] : 0.0;
  __syncthreads();
  if (stopped || row >= dd.M) return;
  const int M = dd.M;
  double f = 0.0;
  const double* __restrict__ xp = dd.Xt + row;
  for (int d = 0; d < dd.D; ++d) f = fma(xp[(size_t)d * dd.Mp], bs[d], f);
  const size_t o = (size_t)c * dd.Mp + row;
  const double res = p.Z[o] - f;
  const double r = sqrt(res * res);
  const long long* off = p.ks_off ? p.ks_off + ((size_t)c * p.T + p.it) * (M + 1) + row : nullptr;
  const long long a0 = off ? off[0] : 0, a1 = off ? off[1] : 0;
  double Lambda = p.lam[o];
  int att = 0, ok = 0, bound = 0;
#pragma unroll 1
  while (att < GIBBS_MAX_ATTEMPTS) {
    double Y, Ua, Ub;
    if (off) {
      if (a0 + att >= a1 || a0 + att >= p.ks_total) { p.stop[c] = 1; break; }  // never past the row's draws (every writer stores 1)
      const double* k3 = p.ks + ((size_t)c * p.ks_total + (size_t)(a0 + att)) * 3;
      Y = k3[0]; Ua = k3[1]; Ub = k3[2];
    } else {
      double U0, U1;
      gibbs_rng(p, c, (uint32_t)row, (uint32_t)p.it, 0x63000000u + 2u * (uint32_t)att, U0, U1);
      Y = normal_first(U0, U1);
      gibbs_rng(p, c, (uint32_t)row, (uint32_t)p.it, 0x63000001u + 2u * (uint32_t)att, Ua, Ub);
    }
    Y = Y * Y;
    Y = 1.0 + (Y - sqrt(Y * (4.0 * r + Y))) / (2.0 * r);
    Lambda = (Ua <= 1.0 / (1.0 + Y)) ? r / Y : r * Y;
    const int v = (Lambda > 4.0 / 3.0) ? gibbs_rightmost(Ub, Lambda) : gibbs_leftmost(Ub, Lambda);
    ++att;
    if (v < 0) bound = 1;
    if (v > 0) { ok = 1; break; }
  }
  if (!ok && att >= GIBBS_MAX_ATTEMPTS) bound = 1;
  if (bound) atomicAdd((unsigned long long*)&p.capped[c], 1ull);
  p.lam[o] = Lambda;
  p.ilam[o] = 1.0 / Lambda;
  if (!(Lambda > 0.0) || !isfinite(Lambda)) { p.stop[c] = 2; p.dead[c] = p.it; }  // (every writer stores the same values)
  if (p.att_out) p.att_out[((size_t)c * p.T + p.it) * M + row] = att;
}
