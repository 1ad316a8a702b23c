// amh.hip.h — gfx950 device code of the component-wise adaptive Metropolis sampler (AMH), reference code/metropolis.py:14-94.
//
// One workgroup of NT threads owns one chain and runs a whole segment of iterations in one launch: every proposal, the
// adaptation and the sample writes, with no host round trip.  Data row n of the chain belongs to thread n mod NT.
//
//   f = X w     on chip in registers (R rows per thread, R*NT >= M), or - R = 0, M too large for that - streamed through two
//               per-chain buffers [Mp] (Chains::rv0 / rv2: the current f and the proposal's f, swapped on acceptance).  Recomputed
//               from w at the start of every segment, so rounding drift of the updates f += delta x_d cannot build up.  A segment
//               may be cut into several launches (bounded work per launch); inside it, f and CurrentLJL are carried over exactly
//               (AmhParams::carry: f in rv0, CurrentLJL in ljl), so the results do not depend on where the launches are cut.
//   w, SD, Accepted[d]   in registers of the thread that owns coordinate j = tid + NT k (k < KW); the per-iteration draws
//               delta_j = z_j SD_j and u_j go through LDS to every thread.
//
// A proposal on coordinate d (metropolis.py:42-64):
//   delta = z SD[d]                             (wNew[d] = w[d] + normal() SD[d])
//   f'    = f + delta x_d                       x_d = column d of Xt [DP][Mp], read coalesced (n < M only: padding never enters)
//   LJL'  = sum_n t_n f'_n - log(1 + exp f'_n) + sum_j LogNormPDF(w'_j)      naive softplus as the reference: inf where exp overflows
//   accept  iff  Ratio > 0  or  Ratio > log(u)  (u read only when Ratio > 0 is false: NaN and -inf read it and reject)
// Every thread forms the same block sum (butterfly, then the wave partials in a fixed order), so every thread takes the same decision
// without a broadcast.  On acceptance the owner moves w_d and the rows move f by the same fma (x_d re-read from cache).
//
// Work per data row and proposal: one exp and one log in fp64 (ocml: roughly 24 + 30 VALU instructions, estimated together with the
// fma, the t f' product and the three adds as AMH_VALU_PER_ROW below) - the bound at large batches; X is shared by all chains and comes
// from cache.
//
// Random streams (the same Philox4x32-10 / u53 / Box-Muller as kernels.hip.h; key = seed, counter = (chain id lo, hi, iteration, block)):
//   block 0x50000000 + (d >> 1)  ->  (U0, U1),  z_d = sqrt(-2 log U0) * (d even ? cos : sin)(2 pi U1)     proposal normal
//   block 0x50001000 + (d >> 1)  ->  (V0, V1),  u_d = d even ? V0 : V1                                    acceptance uniform
// (iteration = IterationNum, 0-based; D <= 256 keeps both ranges inside 0x50000000 .. 0x500010ff.)
// Injected mode (AmhParams::z_in != nullptr) reads z and u from tapes [n][n_iter][D] instead and records, per proposal, the decision
// (bit 0) and whether u was read (bit 1), w and CurrentLJL after every iteration.
#pragma once
#include "kernels.hip.h"
#include "plan.h"  // AMH_MAX_ONCHIP_ROWS

#define AMH_VALU_PER_ROW 60   // ESTIMATE (not counted from the ISA) of the fp64 VALU instructions per data row and proposal: ocml exp ~24,
                              // log ~30, plus the fma, the t f' product, 1 + e^f and the two adds
#define AMH_BLOCK_Z 0x50000000u
#define AMH_BLOCK_U 0x50001000u

struct AmhParams {
  // state between segments, [n][DP] / [n]
  double *w, *sd, *accw, *ljl;
  long long* accepted;
  double *fa, *fb;            // streamed f, [n][Mp] each (R = 0 only)
  // sample mode
  double* samples;            // [n][n_iter - burn_in][D], row k = state after iteration burn_in + k
  unsigned long long seed;
  long long chain_offset;
  // injected mode
  const double *z_in, *u_in;  // [n][n_iter][D]
  double *w_out, *ljl_out;    // [n][n_iter][D], [n][n_iter]
  int8_t* dec_out;            // [n][n_iter][D]
  long long n_iter, burn_in, it0, it1;
  int carry;                  // 0: f and CurrentLJL from w (start of a segment); 1: as the previous launch left them in fa / ljl
};

__device__ __forceinline__ double amh_loglik_row(double t, double f) { return t * f - log(1.0 + exp(f)); }

template <int NT, int R>
__global__ __launch_bounds__(NT) void k_amh(DevData dd, AmhParams p) {
  constexpr int NW = NT / 64, KW = (256 + NT - 1) / NT;
  __shared__ double del_s[256], u_s[256], w_s[256], red[2][NW];
  const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = dd.D, M = dd.M, Mp = dd.Mp, DP = dd.DP;
  const double* __restrict__ Xt = dd.Xt;
  const double* __restrict__ tv = dd.t;
  const bool inj = p.z_in != nullptr;

  auto block_sum = [&](double s, int par) -> double {
    s = wave_sum(s);
    if (NW == 1) return s;
    if (lane == 0) red[par][wave] = s;
    __syncthreads();
    double tot = 0.0;
#pragma unroll
    for (int i = 0; i < NW; ++i) tot += red[par][i];
    return tot;
  };

  double wv[KW], sdv[KW], acv[KW];
#pragma unroll
  for (int k = 0; k < KW; ++k) {
    const int j = tid + NT * k;
    wv[k] = sdv[k] = acv[k] = 0.0;
    if (j < D) {
      wv[k] = p.w[(size_t)c * DP + j]; sdv[k] = p.sd[(size_t)c * DP + j]; acv[k] = p.accw[(size_t)c * DP + j];
      w_s[j] = wv[k];
    }
  }
  long long acc_tot = p.accepted[c];
  __syncthreads();

  // f = X w and the current log joint likelihood (metropolis.py:33-36)
  double f[R > 0 ? R : 1];
  double* fcur = R > 0 ? nullptr : p.fa + (size_t)c * Mp;
  double* fprop = R > 0 ? nullptr : p.fb + (size_t)c * Mp;
  double cur;
  if (p.carry) {
    if constexpr (R > 0) {
      const double* __restrict__ fs = p.fa + (size_t)c * Mp;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int n = tid + NT * r;
        f[r] = n < M ? fs[n] : 0.0;
      }
    }
    cur = p.ljl[c];
  } else {
    double s = 0.0;
    if constexpr (R > 0) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int n = tid + NT * r;
        double fr = 0.0;
        if (n < M) {
          for (int d = 0; d < D; ++d) fr = fma(Xt[(size_t)d * Mp + n], w_s[d], fr);
          s += amh_loglik_row(tv[n], fr);
        }
        f[r] = fr;
      }
    } else {
      for (int n = tid; n < M; n += NT) {
        double fr = 0.0;
        for (int d = 0; d < D; ++d) fr = fma(Xt[(size_t)d * Mp + n], w_s[d], fr);
        fcur[n] = fr;
        s += amh_loglik_row(tv[n], fr);
      }
    }
#pragma unroll
    for (int k = 0; k < KW; ++k)
      if (tid + NT * k < D) s += dd.log_prior_const - 0.5 * dd.inv_alpha * wv[k] * wv[k];
    cur = block_sum(s, 0);
  }

  const long long S = p.n_iter - p.burn_in;
  const unsigned long long gid = (unsigned long long)(p.chain_offset + c);
  for (long long it = p.it0; it < p.it1; ++it) {
    __syncthreads();  // every thread is done with the previous iteration's draws (and with red)
#pragma unroll
    for (int k = 0; k < KW; ++k) {
      const int j = tid + NT * k;
      if (j >= D) continue;
      double z, u;
      if (inj) {
        const size_t o = ((size_t)c * p.n_iter + it) * D + j;
        z = p.z_in[o]; u = p.u_in[o];
      } else {
        double U0, U1, V0, V1;
        rng_block(p.seed, gid, (uint32_t)it, AMH_BLOCK_Z + (uint32_t)(j >> 1), U0, U1);
        rng_block(p.seed, gid, (uint32_t)it, AMH_BLOCK_U + (uint32_t)(j >> 1), V0, V1);
        z = normal_of_pair(U0, U1, j & 1);
        u = (j & 1) ? V1 : V0;
      }
      del_s[j] = z * sdv[k];
      u_s[j] = u;
    }
    __syncthreads();

    for (int d = 0; d < D; ++d) {
      const double delta = del_s[d];
      const double* __restrict__ xd = Xt + (size_t)d * Mp;
      double sp = 0.0;
      if constexpr (R > 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int n = tid + NT * r;
          if (n < M) sp += amh_loglik_row(tv[n], fma(delta, xd[n], f[r]));
        }
      } else {
        for (int n = tid; n < M; n += NT) {
          const double fp = fma(delta, xd[n], fcur[n]);
          fprop[n] = fp;
          sp += amh_loglik_row(tv[n], fp);
        }
      }
#pragma unroll
      for (int k = 0; k < KW; ++k) {
        const int j = tid + NT * k;
        if (j < D) {
          const double v = j == d ? wv[k] + delta : wv[k];
          sp += dd.log_prior_const - 0.5 * dd.inv_alpha * v * v;
        }
      }
      const double prop = block_sum(sp, d & 1);
      const double ratio = prop - cur;
      bool acc = ratio > 0.0, uread = false;
      if (!acc) {
        uread = true;
        acc = ratio > log(u_s[d]);
      }
      if (inj && tid == 0) p.dec_out[((size_t)c * p.n_iter + it) * D + d] = (int8_t)((acc ? 1 : 0) | (uread ? 2 : 0));
      if (acc) {
        cur = prop;
        ++acc_tot;
#pragma unroll
        for (int k = 0; k < KW; ++k)
          if (tid + NT * k == d) { wv[k] += delta; acv[k] += 1.0; }
        if constexpr (R > 0) {
#pragma unroll
          for (int r = 0; r < R; ++r) {
            const int n = tid + NT * r;
            if (n < M) f[r] = fma(delta, xd[n], f[r]);
          }
        } else {
          double* tmp = fcur; fcur = fprop; fprop = tmp;
        }
      }
    }

    // per-iteration record / saved sample (metropolis.py:67-68; row 0 = state after iteration BurnIn)
#pragma unroll
    for (int k = 0; k < KW; ++k) {
      const int j = tid + NT * k;
      if (j >= D) continue;
      if (inj) p.w_out[((size_t)c * p.n_iter + it) * D + j] = wv[k];
      else if (it >= p.burn_in) p.samples[((size_t)c * S + (it - p.burn_in)) * D + j] = wv[k];
    }
    if (inj && tid == 0) p.ljl_out[(size_t)c * p.n_iter + it] = cur;
    // adaptation (metropolis.py:71-90), iteration 0 included: its window holds one proposal per coordinate, later ones 100
    if (it % 100 == 0 && it < p.burn_in) {
      const double proposed = it == 0 ? 1.0 : 100.0;
#pragma unroll
      for (int k = 0; k < KW; ++k) {
        const double ar = acv[k] / proposed;
        if (ar > 0.5) sdv[k] *= 1.2;
        else if (ar < 0.2) sdv[k] *= 0.8;
        acv[k] = 0.0;
      }
    }
  }

#pragma unroll
  for (int k = 0; k < KW; ++k) {
    const int j = tid + NT * k;
    if (j < D) { p.w[(size_t)c * DP + j] = wv[k]; p.sd[(size_t)c * DP + j] = sdv[k]; p.accw[(size_t)c * DP + j] = acv[k]; }
  }
  // f for the next launch of the segment, in fa (each thread writes the rows it reads back: no barrier needed)
  if constexpr (R > 0) {
    double* __restrict__ fs = p.fa + (size_t)c * Mp;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int n = tid + NT * r;
      if (n < M) fs[n] = f[r];
    }
  } else if (fcur != p.fa + (size_t)c * Mp) {
    for (int n = tid; n < M; n += NT) fprop[n] = fcur[n];   // (fprop is fa here)
  }
  if (tid == 0) { p.accepted[c] = acc_tot; p.ljl[c] = cur; }
}

// Rows per thread of the on-chip variants: NT = 64 (one wavefront per chain) when there are enough chains to fill the chip and M is
// small, NT = 256 otherwise; R = 0 streams f.
#define AMH_SWITCH(NT, R, ...)                                                                                  \
  do {                                                                                                          \
    if ((NT) == 64) {                                                                                           \
      if ((R) <= 4) { constexpr int NT_ = 64, R_ = 4; __VA_ARGS__; }                                            \
      else if ((R) <= 8) { constexpr int NT_ = 64, R_ = 8; __VA_ARGS__; }                                       \
      else { constexpr int NT_ = 64, R_ = 16; __VA_ARGS__; }                                                    \
    } else if ((R) == 0) { constexpr int NT_ = 256, R_ = 0; __VA_ARGS__; }                                      \
    else if ((R) <= 2) { constexpr int NT_ = 256, R_ = 2; __VA_ARGS__; }                                        \
    else if ((R) <= 4) { constexpr int NT_ = 256, R_ = 4; __VA_ARGS__; }                                        \
    else if ((R) <= 8) { constexpr int NT_ = 256, R_ = 8; __VA_ARGS__; }                                        \
    else if ((R) <= 16) { constexpr int NT_ = 256, R_ = 16; __VA_ARGS__; }                                      \
    else if ((R) <= 32) { constexpr int NT_ = 256, R_ = 32; __VA_ARGS__; }                                      \
    else { constexpr int NT_ = 256, R_ = 48; __VA_ARGS__; }                                                     \
  } while (0)
// Work bound of one launch, in (chain, proposal, data row) evaluations: 2^34, ~0.15 s at the 1.2e11 / s measured at 8192 chains x D 64
// x M 10 000 (profiles/amh_bench.jsonl).  A segment whose work exceeds it runs as several launches (AmhParams::carry).
#define AMH_LAUNCH_ROWS (1LL << 34)
