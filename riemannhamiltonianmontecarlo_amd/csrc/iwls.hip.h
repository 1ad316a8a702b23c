// iwls.hip.h — the reference's IWLS Metropolis-Hastings sampler (code/iwls.py:13-89) on gfx950, on the helpers of kernels.hip.h.
// D <= 64: one wavefront per chain, lane = dimension.
//
// Per chain, with the point record of kernels.hip.h (Rec: w, grad = X'(t - p) - w/alpha, L L' = G = X'WX + I/alpha, Ginv, ljl, hld):
//   mean          m(w) = w + Ginv grad                      (the reference's cov X'W z, iwls.py:33-35,59-61, without 1/W)
//   proposal      w' = m(w) + L^-T z,  z ~ N(0, I)          (multivariate_normal(current_mean, current_cov), :45)
//   log q(x | w)  = l(w) - |L'(x - m(w))|^2 / 2,  l(w) = -sum log diag chol(Ginv + 1e-6 I) (compat, :64,:68) or hld
//   ratio         LJL(w') + log q(w | w') - LJL(w) - log q(w' | w)   (:73)
// compat: a proposal with a row whose W_j = p_j (1 - p_j) is 0 or has a non-finite 1/W_j (p_j = 1/(1 + exp(-f_j)) in fp64) gets
// ratio = NaN, the reference's 0/0 (inv_W = eye/W, :56), and is rejected.  A record at w' that is not positive definite is rejected
// in both modes (ratio = NaN).  Accept iff ratio > 0 or ratio > log u; u is read only when ratio > 0 is false (:76).
//
// One iteration is: k_iwls_begin, the point evaluation at w' (eval_point_phases mode 1: row pass, assembly on the fp64 or int8 matrix
// cores, factor / inverse), compat only k_iwls_ljit on trj.Ginv and k_iwls_sat, then k_iwls_end.
// Random streams (kernels.hip.h header): proposal normals from draw_normals (blocks d/2, Box-Muller), acceptance uniform from rng_u_acc
// (RM_BLOCK_LEN_ACC); counter iteration = i, key (seed, chain_offset + c).  The replay entry point reads w' and u from tapes instead.
#pragma once
#include "kernels.hip.h"

struct IwlsParams {
  unsigned long long seed;
  long long chain_offset;
  long long it;            // iteration i
  long long burn_in, S;    // samples [n][S][D]: row k = w after iteration burn_in + k
  double* samples;         // or nullptr
  long long T;             // replay: iterations of the tapes and records
  const double* w_prop;    // replay: proposals [n][T][D] (nullptr: Philox)
  const double* u_in;      // replay: uniforms [n][T] (NaN where the reference drew none)
  double *w_out, *mean_out, *ljl_out, *ratio_out;  // replay records after every iteration, [n][T][D] / [n][T], or nullptr
  int8_t* dec_out;         // [n][T]: bit 0 accepted, bit 1 u read, bit 2 saturated
  int compat;
  double *lq_cur, *lq_trj; // [n] l() of the records cur / trj (compat: the jittered term; unused otherwise)
  int* sat;                // [n] the proposal of this iteration is saturated (k_iwls_sat)
  long long* nsat;         // [n] saturated proposals so far
  double* mcur;            // [n][DP] m(cur.w) of this iteration
};

// m_lane = w_lane + sum_j Ginv[j][lane] g_j (Ginv symmetric; gs: the gradient in LDS).  The same sums in the same order for cur
// (k_iwls_begin) and trj (k_iwls_end), so the mean of an accepted proposal is the one the next iteration recomputes.
__device__ __forceinline__ double iwls_mean(const double* __restrict__ Gi, const double* gs, double w, int D, int DP, int lane) {
  return w + symv64(Gi, D, DP, lane, [&](int j) { return gs[j]; });
}

// |L' d|^2 for d in LDS (L lower)
__device__ __forceinline__ double iwls_quad(const double* __restrict__ L, const double* ds, int D, int DP, int lane) {
  const double y = ltv64(L, D, DP, lane, [&](int i) { return ds[i]; });
  return wave_sum(lane < D ? y * y : 0.0);
}

// proposal, and LJL(w) + log q(w' | w) of the current state into Hcur
__global__ __launch_bounds__(64) void k_iwls_begin(int D, int DP, Chains ch, IwlsParams p) {
  __shared__ double gs[64], zs[64], ds[64];
  const int c = blockIdx.x, lane = threadIdx.x;
  const bool in = lane < D;
  const size_t o = (size_t)c * DP;
  gs[lane] = in ? ch.cur.grad[o + lane] : 0.0;
  __syncthreads();
  const double m = iwls_mean(ch.cur.Ginv + o * DP, gs, in ? ch.cur.w[o + lane] : 0.0, D, DP, lane);
  const double* __restrict__ Lc = ch.cur.L + o * DP;
  double wp;
  if (p.w_prop) {
    wp = in ? p.w_prop[((size_t)c * p.T + p.it) * D + lane] : 0.0;
  } else {
    IterParams ip{};
    ip.seed = p.seed;
    ip.chain_offset = p.chain_offset;
    draw_normals(ip, c, p.it, D, lane, zs);
    // x = L^-T z by back substitution (L' upper triangular): lane i holds the residual r_i, then x_i
    double r = in ? zs[lane] : 0.0;
    for (int j = D - 1; j >= 0; --j) {
      const double xj = rdlane(r, j) / Lc[(size_t)j * DP + j];
      if (lane == j) r = xj;
      else if (lane < j) r = fma(-Lc[(size_t)j * DP + lane], xj, r);
    }
    wp = m + r;
  }
  ds[lane] = in ? wp - m : 0.0;
  __syncthreads();
  const double quad = iwls_quad(Lc, ds, D, DP, lane);
  const double lq = p.compat ? p.lq_cur[c] : ch.cur.hld[c];
  if (in) {
    ch.trj.w[o + lane] = wp;
    p.mcur[o + lane] = m;
  }
  if (lane == 0) {
    ch.Hcur[c] = ch.cur.ljl[c] + (lq - 0.5 * quad);
    ch.status[c] = 0;
    ch.phase[c] = 1;
    p.sat[c] = 0;
  }
}

// compat: out[c] = -sum log diag chol(Ginv + 1e-6 I)   (iwls.py:64,68), packed LDS image as in k_factor_full
template <int NB>
__global__ __launch_bounds__(64) void k_iwls_ljit(int D, int DP, const double* __restrict__ Ginv, double* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) double A[RM_PK_DOUBLES];
  const int c = blockIdx.x, lane = threadIdx.x;
  load_mat_lds<true>(A, Ginv + (size_t)c * DP * DP, D, DP, lane);
  if (lane < D) A[rm_row<true>(lane) + lane] += 1e-6;
  __syncthreads();
  double rdiag;
  (void)chol_lds_blk<NB, true>(A, D, lane, rdiag);  // (not positive definite: NaN, and the proposal is rejected)
  const double l = wave_sum(lane < D ? log(rdiag) : 0.0);  // rdiag = 1 / L_jj
  if (lane == 0) out[c] = l;
}

// compat: sat[c] = 1 where some row of f = X w' has W_j == 0 or a non-finite 1/W_j.  f in fp64 from Xt (the int8 row pass keeps no
// fp64 v).  A block is IWLS_SAT_ROWS rows x IWLS_SAT_CH chains: every X value read serves IWLS_SAT_CH chains, w' comes from LDS.
#define IWLS_SAT_ROWS 256
#define IWLS_SAT_CH 32
__global__ __launch_bounds__(IWLS_SAT_ROWS) void k_iwls_sat(DevData dd, int n, const double* __restrict__ w, int* __restrict__ sat) {
  __shared__ __attribute__((aligned(16))) double ws[64 * IWLS_SAT_CH];  // [d][chain]
  const int c0 = blockIdx.y * IWLS_SAT_CH;
  const int D = dd.D, DP = dd.DP;
  for (int k = threadIdx.x; k < D * IWLS_SAT_CH; k += IWLS_SAT_ROWS) {
    const int d = k / IWLS_SAT_CH, j = k % IWLS_SAT_CH;
    ws[k] = (c0 + j < n) ? w[(size_t)(c0 + j) * DP + d] : 0.0;
  }
  __syncthreads();
  const int row = blockIdx.x * IWLS_SAT_ROWS + threadIdx.x;
  if (row >= dd.M) return;
  double f[IWLS_SAT_CH];
#pragma unroll
  for (int j = 0; j < IWLS_SAT_CH; ++j) f[j] = 0.0;
  const double* __restrict__ xp = dd.Xt + row;
  for (int d = 0; d < D; ++d) {
    const double x = xp[(size_t)d * dd.Mp];
#pragma unroll
    for (int j = 0; j < IWLS_SAT_CH; ++j) f[j] = fma(x, ws[d * IWLS_SAT_CH + j], f[j]);
  }
#pragma unroll
  for (int j = 0; j < IWLS_SAT_CH; ++j) {
    const double pj = 1.0 / (1.0 + exp(-f[j]));
    const double Wj = pj * (1.0 - pj);
    if ((Wj == 0.0 || !isfinite(1.0 / Wj)) && c0 + j < n) sat[c0 + j] = 1;  // (every writer stores the same value)
  }
}

// ratio, decision, record copy, counters and outputs, once the record at w' is evaluated
__global__ __launch_bounds__(64) void k_iwls_end(int D, int DP, Chains ch, IwlsParams p) {
  __shared__ double gs[64], ds[64];
  const int c = blockIdx.x, lane = threadIdx.x;
  const bool in = lane < D;
  const size_t o = (size_t)c * DP;
  const double wp = in ? ch.trj.w[o + lane] : 0.0, w = in ? ch.cur.w[o + lane] : 0.0;
  gs[lane] = in ? ch.trj.grad[o + lane] : 0.0;
  __syncthreads();
  const double mp = iwls_mean(ch.trj.Ginv + o * DP, gs, wp, D, DP, lane);
  ds[lane] = in ? w - mp : 0.0;
  __syncthreads();
  const double quad = iwls_quad(ch.trj.L + o * DP, ds, D, DP, lane);
  const double lq = p.compat ? p.lq_trj[c] : ch.trj.hld[c];
  const double ljl_p = ch.trj.ljl[c], ljl_c = ch.cur.ljl[c];
  double ratio = ljl_p + (lq - 0.5 * quad) - ch.Hcur[c];
  const bool saturated = p.compat && p.sat[c] != 0;
  if ((ch.status[c] & 1) || saturated) ratio = __builtin_nan("");
  const bool u_read = !(ratio > 0.0);
  bool accept = !u_read;
  if (u_read) {
    double u;
    if (p.w_prop) {
      u = p.u_in[(size_t)c * p.T + p.it];
    } else {
      u = rng_u_acc(p.seed, (unsigned long long)(p.chain_offset + c), (uint32_t)p.it);
    }
    accept = ratio > log(u);
  }
  const double m_out = accept ? mp : (in ? p.mcur[o + lane] : 0.0);
  const double w_new = accept ? wp : w;
  __syncthreads();
  if (accept) {
    copy_rec(ch.cur, ch.trj, c, D, DP, lane);
    if (lane == 0 && p.compat) p.lq_cur[c] = p.lq_trj[c];
  }
  if (p.samples && p.it >= p.burn_in && in) p.samples[((size_t)c * p.S + (size_t)(p.it - p.burn_in)) * D + lane] = w_new;
  if (p.w_out) {
    const size_t r = (size_t)c * p.T + p.it;
    if (in) {
      p.w_out[r * D + lane] = w_new;
      if (p.mean_out) p.mean_out[r * D + lane] = m_out;
    }
    if (lane == 0) {
      if (p.ljl_out) p.ljl_out[r] = accept ? ljl_p : ljl_c;
      if (p.ratio_out) p.ratio_out[r] = ratio;
      if (p.dec_out) p.dec_out[r] = (int8_t)((accept ? 1 : 0) | (u_read ? 2 : 0) | (saturated ? 4 : 0));
    }
  }
  if (lane == 0) {
    ch.Hprop[c] = ratio;
    if (accept) ch.accepted[c] += 1;
    if (saturated) p.nsat[c] += 1;
    ch.iter[c] = p.it + 1;
    ch.phase[c] = 0;
  }
}
