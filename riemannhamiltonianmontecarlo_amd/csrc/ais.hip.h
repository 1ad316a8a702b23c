// ais.hip.h — annealed importance sampling with tempered fixed-metric HMC (include/rmhmc_ais.h).
//
// Tempered target: LJL_beta = beta loglik + logprior, grad_beta = beta grad_lik - w / alpha.  The row pass writes the likelihood's
// gradient and log-likelihood partials (gpart, ljl_part) apart from the prior, so tempering costs no O(M D) kernel: one global step is
//   k_phmc_head      as it is: it reads the records' gradient, which is stored tempered, and nothing else that depends on beta
//   k_rowpass<RP_G>  as it is
//   k_tphmc_tail     k_phmc_tail with tphmc_finish_eval in place of hmc_finish_eval; the chain's loglik goes beside its ljl (ll[c] is
//                    the current point's: written when a proposal that moved is accepted)
// and the initial evaluation is the row pass plus k_tphmc_init, which inside rmhmc_ais_run also forms loglik0 of the stage and adds
// (beta_k - beta_{k-1}) loglik0 to logw.
//
// beta = 1 reproduces hmc_finish_eval to the bit.  What that function compiles to under the contraction mode of kernels.hip.h is
//   grad = fma(-inv_alpha, w, gsum)      part += fma(inv_alpha, (w w)(-0.5), log_prior_const)      part += ljl_part[b]
// and this header writes exactly that with explicit fma() and contraction off, with beta gsum and beta ljl_part[b] (1 x is exact) in
// place of gsum and ljl_part[b].  tests/test_gpu_ais.py holds the two to bit equality.  The log-likelihood is a second wave_sum over the
// lanes' sums of ljl_part alone, in the same order.
//
// k_ais_prior: one wavefront per chain, w = sqrt(alpha) z with z from draw_normals at iteration counter RMHMC_AIS_PRIOR_ITER.
//
// Weights (the partial of include/rmhmc_ais.h), three kernels, no atomics, every order fixed by n alone:
//   k_ais_max   grid: blocks of ais_plan x 256 threads.  NaN entries are counted and left out; the block's maximum of the others, the
//               counts of used and NaN entries -> blk [nblocks][3]
//   k_ais_sums  the same grid.  Every block first takes the global maximum a from blk (the same value in each); thread t adds
//               exp(lw - a) and exp(2 (lw - a)) of its entries t, t + 256, ... into the sum_pairs of sums.hip.h; thread 0
//               adds the 256 pairs in thread order -> sums [nblocks][4]
//   k_ais_fin   one thread: the blocks in block order -> partial [5]
// a = -inf (every used entry -inf, or none used) makes every term 0 without reading anything else; no index depends on the data.
#pragma once
#include "../../include/rmhmc_ais.h"  // RMHMC_AIS_PRIOR_ITER
#include "phmc.hip.h"
#include "sums.hip.h"  // sum_pair, block_rows, SUM_NEG_INF
#include "ais.h"       // ais_plan

#pragma clang fp contract(off)

// LJL_beta, grad_beta of the row pass's partials into trj.grad / trj.ljl; returns loglik (every lane), NaN where trj.w is not finite
__device__ __forceinline__ double tphmc_finish_eval(const DevData& dd, const Chains& ch, int c, int lane, int nsplit, double beta) {
  const int D = dd.D, DP = dd.DP;
  double part = 0.0, lik = 0.0;
  int w_bad = 0;
  for (int d = lane; d < D; d += 64) {
    const double wl = ch.trj.w[(size_t)c * DP + d];
    ch.trj.grad[(size_t)c * DP + d] = fma(-dd.inv_alpha, wl, beta * plane_sum(ch.gpart, nsplit, ch.n, c, DP, d));
    part = part + fma(dd.inv_alpha, (wl * wl) * -0.5, dd.log_prior_const);
    w_bad |= !isfinite(wl);
  }
  for (int b = lane; b < nsplit; b += 64) {
    const double x = ch.ljl_part[(size_t)c * nsplit + b];
    part = part + beta * x;
    lik = lik + x;
  }
  const double ljl = wave_sum(part);
  const double ll = wave_sum(lik);
  if (lane == 0) ch.trj.ljl[c] = ljl;
  // a position that is not finite has f = +-inf or NaN on every row its column reaches, and t f - log(1 + exp f) is 0 x inf or inf - inf
  // there: loglik is NaN (include/rmhmc_ais.h).  The row pass of D <= 64 reports an f above 709.78 as -inf whatever else the split holds
  // (kernels.hip.h), which is the reference's value for a finite f and hid the NaN of an infinite one; large_d.hip.h keeps it.
  return __ballot(w_bad) ? __builtin_nan("") : ll;
}

// initial evaluation at trj.w under beta: trj -> cur, ll[c] = loglik; ll0 | nullptr: a copy that the stepping does not overwrite;
// logw | nullptr: logw[c] += dbeta loglik, NaN where loglik is not finite (the weight update of a stage of rmhmc_ais_run)
__global__ __launch_bounds__(64) void k_tphmc_init(DevData dd, Chains ch, int nsplit, double beta, double* __restrict__ ll,
                                                   double* __restrict__ ll0, double* __restrict__ logw, double dbeta) {
  const int c = blockIdx.x, lane = threadIdx.x;
  const double l = tphmc_finish_eval(dd, ch, c, lane, nsplit, beta);
  __syncthreads();
  hmc_copy(ch.cur, ch.trj, c, dd.D, dd.DP, lane);
  if (lane == 0) {
    ll[c] = l;
    if (ll0) ll0[c] = l;
    if (logw) logw[c] = isfinite(l) ? logw[c] + dbeta * l : __builtin_nan("");  // (a loglik that is not finite: the chain has failed)
  }
}

// k_phmc_tail under beta (see there); ll [n]: loglik of the current point of every chain
template <int NDB>
__global__ __launch_bounds__(256) void k_tphmc_tail(DevData dd, Chains ch, IterParams ip, PhmcMass pm, double eps, int nsplit, double beta,
                                                    double* __restrict__ ll) {
  using S = PhmcShape<NDB>;
  constexpr int DP = S::DP, VLD = S::VLD;
  extern __shared__ double phmc_lds[];
  __shared__ int flag[16];
  double* mat = phmc_lds;
  double* vs = mat + S::MAT;
  const int D = dd.D;
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const int c0 = blockIdx.x * 16;
  double llp[4] = {0.0, 0.0, 0.0, 0.0};  // loglik at trj.w of the wavefront's four chains, where this launch has evaluated it
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const int c = c0 + wv + 4 * jj;
    if (c < ch.n && ch.phase[c] == 1) llp[jj] = tphmc_finish_eval(dd, ch, c, lane, nsplit, beta);
  }
  __syncthreads();
  int ending = 0;
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const int j = wv + 4 * jj, c = c0 + j;
    double* v = vs + j * VLD;
    int f = 0;
    if (c < ch.n) {
      const int ph = ch.phase[c];
      if (ph == 1) {
        const int left = ch.steps_left[c] - 1;
        if (!(ch.status[c] & 2))
          for (int d = lane; d < D; d += 64) ch.p[(size_t)c * DP + d] = fma(eps * 0.5, ch.trj.grad[(size_t)c * DP + d], ch.p[(size_t)c * DP + d]);
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) { ch.steps_left[c] = left; ch.steps_done[c] += 1; }
        if (left == 0) f = PHMC_STEP;
      } else if (ph == 2) {
        f = PHMC_STEP | PHMC_NAN;  // (PHMC_NAN here: a trajectory of zero steps - the proposal is the current point, ll[c] stays)
      }
    }
    for (int d = lane; d < DP; d += 64) v[d] = (f && d < D) ? ch.p[(size_t)c * DP + d] : 0.0;
    if (lane == 0) flag[j] = f;
    ending |= f;
  }
  if (!__syncthreads_or(ending)) return;
  phmc_product<NDB>(pm.Minv, mat, vs, tid);  // Mass^-1 p of the proposals
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const int j = wv + 4 * jj, c = c0 + j;
    const double* v = vs + j * VLD;
    const int f = flag[j];
    if (!f) continue;
    const long long it = ch.iter[c];
    double kin = 0.0;
    for (int d = lane; d < D; d += 64) { const double pl = ch.p[(size_t)c * DP + d]; kin = fma(pl, v[d], kin); }
    const double Hc = ch.Hcur[c];
    const double Hp = -ch.trj.ljl[c] + 0.5 * wave_sum(kin);
    const double ratio = -Hp + Hc;
    const bool failed = (ch.status[c] & 2) || !isfinite(Hc) || !isfinite(Hp);
    const bool accept = !failed && mh_accept(ratio, draw_u_acc(ip, c, c, it));
    if (accept) hmc_copy(ch.cur, ch.trj, c, D, DP, lane);
    __builtin_amdgcn_wave_barrier();  // (a lane reads back only what it wrote itself)
    if (lane == 0) {
      if (failed) ch.status[c] |= 2;
      if (accept && !(f & PHMC_NAN)) ll[c] = llp[jj];
    }
    close_transition(D, DP, ch, ip, c, c, lane, it, Hp, accept);
  }
}

// exact draws from the prior N(0, alpha I): out[c * ld + d] = sqrt_alpha z_d
__global__ __launch_bounds__(64) void k_ais_prior(int D, unsigned long long seed, long long chain_offset, double sqrt_alpha,
                                                  double* __restrict__ out, int ld) {
  __shared__ double zs[RM_DMAX];
  const int c = blockIdx.x, lane = threadIdx.x;
  IterParams ip{};
  ip.seed = seed;
  ip.chain_offset = chain_offset;
  draw_normals(ip, c, (long long)RMHMC_AIS_PRIOR_ITER, D, lane, zs);
  for (int d = lane; d < D; d += 64) out[(size_t)c * ld + d] = sqrt_alpha * zs[d];
}

__global__ __launch_bounds__(256) void k_ais_max(const double* __restrict__ lw, size_t n, size_t per_block, double* __restrict__ blk) {
  __shared__ double r_a[256], r_m[256], r_n[256];
  const int tid = threadIdx.x;
  const block_range rg = block_rows(blockIdx.x, per_block, n);
  double a = SUM_NEG_INF, m = 0.0, nn = 0.0;
  for (size_t i = rg.begin + tid; i < rg.end; i += 256) {
    const double x = lw[i];
    if (x != x) { nn += 1.0; continue; }
    m += 1.0;
    a = x > a ? x : a;
  }
  r_a[tid] = a; r_m[tid] = m; r_n[tid] = nn;
  __syncthreads();
  if (tid == 0) {
    for (int t = 1; t < 256; ++t) {
      a = r_a[t] > a ? r_a[t] : a;
      m += r_m[t];
      nn += r_n[t];
    }
    blk[3 * (size_t)blockIdx.x] = a;
    blk[3 * (size_t)blockIdx.x + 1] = m;
    blk[3 * (size_t)blockIdx.x + 2] = nn;
  }
}

__global__ __launch_bounds__(256) void k_ais_sums(const double* __restrict__ lw, size_t n, size_t per_block, const double* __restrict__ blk,
                                                  int nblocks, double* __restrict__ sums) {
  __shared__ sum_pair r[2][256];  // (r[0][].s first carries the threads' maxima)
  const int tid = threadIdx.x;
  double a = SUM_NEG_INF;
  for (int b = tid; b < nblocks; b += 256) a = blk[3 * (size_t)b] > a ? blk[3 * (size_t)b] : a;
  r[0][tid].s = a;
  __syncthreads();
  for (int t = 0; t < 256; ++t) a = r[0][t].s > a ? r[0][t].s : a;  // (a maximum: any order gives the same value)
  __syncthreads();
  const block_range rg = block_rows(blockIdx.x, per_block, n);
  sum_pair s1 = {}, s2 = {};
  if (a > SUM_NEG_INF) {
    for (size_t i = rg.begin + tid; i < rg.end; i += 256) {
      const double x = lw[i];
      if (x != x) continue;
      const double dx = x - a;
      s1.add(exp(dx));
      s2.add(exp(2.0 * dx));
    }
  }
  r[0][tid] = s1; r[1][tid] = s2;
  __syncthreads();
  if (tid == 0) {
    for (int t = 1; t < 256; ++t) {
      s1.add(r[0][t]);
      s2.add(r[1][t]);
    }
    double* out = sums + 4 * (size_t)blockIdx.x;
    out[0] = s1.s; out[1] = s1.e; out[2] = s2.s; out[3] = s2.e;
  }
}

__global__ __launch_bounds__(64) void k_ais_fin(const double* __restrict__ blk, const double* __restrict__ sums, int nblocks,
                                                double* __restrict__ partial) {
  if (threadIdx.x != 0) return;
  double a = SUM_NEG_INF, m = 0.0, nn = 0.0;
  sum_pair s1 = {}, s2 = {};
  for (int b = 0; b < nblocks; ++b) {
    const double* in = sums + 4 * (size_t)b;
    a = blk[3 * (size_t)b] > a ? blk[3 * (size_t)b] : a;
    m += blk[3 * (size_t)b + 1];
    nn += blk[3 * (size_t)b + 2];
    s1.add(sum_pair{in[0], in[1]});
    s2.add(sum_pair{in[2], in[3]});
  }
  partial[0] = m;
  partial[1] = nn;
  partial[2] = a;
  partial[3] = s1.value();
  partial[4] = s2.value();
}
