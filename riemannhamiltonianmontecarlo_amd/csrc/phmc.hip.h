// phmc.hip.h — HMC with a fixed dense mass matrix shared by all chains (include/rmhmc_phmc.h).
//
// One transition is plain HMC (kernels.hip.h: k_hmc_begin / pre / post / end, code/hmc.py:38-84) with Mass = Lm Lm' in place of
// the identity:  p = Lm z,  H = -LJL + p' Mass^-1 p / 2,  w += eps Mass^-1 p.  One global step is three launches:
//   k_phmc_head   chains between transitions start one (draws, p = Lm z, H_cur, trajectory length); every chain in a trajectory
//                 takes the first momentum half step and the position step
//   k_rowpass<RP_G>  gradient and log-joint partials at the new position (the launch plain HMC uses, untouched)
//   k_phmc_tail   hmc_finish_eval, second half step, step counters; chains whose trajectory is over: kinetic term, decision,
//                 sample, bookkeeping (k_hmc_end)
// Records: cur / trj .w .grad .ljl and p, as plain HMC.  Random streams: those of k_hmc_begin / k_hmc_end.
//
// The products with the shared matrices (Lm z, Mass^-1 p) are [DP x DP] x [DP x 16 chains] on v_mfma_f64_16x16x4_f64: a
// workgroup of four wavefronts owns 16 consecutive chains, the matrix is staged in LDS once per workgroup and product (in column
// blocks of 32 for D > 64), the 16 vectors sit in LDS as the B operand, and wavefront v accumulates the 16-row blocks v, v + 4, ...
// of the result (lane map of the fp64 MFMA: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15], result
// row (lane >> 4) + 4 r, column lane & 15 in element r).  A chain is a COLUMN of the product, so a chain that carries NaN or inf
// cannot reach its neighbours.  The per-chain parts run one chain per wavefront, four chains after one another, in the lane order
// of the plain HMC kernels (lane d owns d, d + 64, ...; fma chain; wave_sum), so that with the identity images - exact zeros and
// ones - every sum, and with it every position, momentum, Hamiltonian and decision, is plain HMC's bit for bit.  The half steps and
// the position step are explicit fma(): that is what the compiler contracts them to in k_hmc_pre / k_hmc_post, and this header must
// not depend on the contraction mode it is included under (fused_small.hip.h switches it off for the rest of the translation unit).
#pragma once
#include "kernels.hip.h"

struct PhmcMass {
  const double* Lm;    // [DP][DP] row-major, zero padded: lower Cholesky factor of the mass matrix
  const double* Minv;  // [DP][DP] its inverse (symmetric)
};

// NDB = DP / 16: 1..4 (D <= 64) or 8, 12, 16 (large-D contexts, DP a multiple of 64)
template <int NDB>
struct PhmcShape {
  static constexpr int DP = 16 * NDB;
  static constexpr int KB = DP <= 64 ? DP : 32;  // columns of the matrix held in LDS at a time
  static constexpr int LD = KB + 4;              // (rows 4 doubles apart modulo 32: the A fragments of one MFMA spread over the banks)
  static constexpr int VLD = DP + 4;
  static constexpr int MAT = DP * LD;
  static constexpr int LDS_DOUBLES = MAT + 16 * VLD;
};
template <int NDB>
constexpr size_t phmc_lds_bytes() { return sizeof(double) * PhmcShape<NDB>::LDS_DOUBLES; }

// vs[j][.] <- Mg vs[j][.] for the 16 chains j of the workgroup (vs: [16][VLD], rows of DP entries).  Every thread of the 256 calls it;
// the vectors must have been written before the call (no barrier needed in between) and hold the result after it.
template <int NDB>
__device__ __forceinline__ void phmc_product(const double* __restrict__ Mg, double* mat, double* vs, int tid) {
  using S = PhmcShape<NDB>;
  constexpr int DP = S::DP, KB = S::KB, LD = S::LD, VLD = S::VLD, NI = (NDB + 3) / 4;
  const int wv = tid >> 6, lane = tid & 63, rr = lane >> 4, ci = lane & 15;
  d4 acc[NI];
#pragma unroll
  for (int ii = 0; ii < NI; ++ii) acc[ii] = (d4){0.0, 0.0, 0.0, 0.0};
  for (int kb = 0; kb < DP; kb += KB) {
    if (kb) __syncthreads();  // the previous column block has been consumed
    for (int idx = tid; idx < DP * KB; idx += 256) {
      const int r = idx / KB, k = idx - r * KB;
      mat[r * LD + k] = Mg[(size_t)r * DP + kb + k];
    }
    __syncthreads();
#pragma unroll 4
    for (int k0 = 0; k0 < KB; k0 += 4) {
      const double b = vs[ci * VLD + kb + k0 + rr];
#pragma unroll
      for (int ii = 0; ii < NI; ++ii) {
        const int I = wv + 4 * ii;
        if (I < NDB) acc[ii] = __builtin_amdgcn_mfma_f64_16x16x4f64(mat[(16 * I + ci) * LD + k0 + rr], b, acc[ii], 0, 0, 0);
      }
    }
  }
  __syncthreads();  // every wavefront has read the vectors: the result goes in their place
#pragma unroll
  for (int ii = 0; ii < NI; ++ii) {
    const int I = wv + 4 * ii;
    if (I < NDB) {
#pragma unroll
      for (int r = 0; r < 4; ++r) vs[ci * VLD + 16 * I + rr + 4 * r] = acc[ii][r];
    }
  }
  __syncthreads();
}

// per-chain flags of a launch, in LDS
#define PHMC_BEGUN 1  // the chain has started a transition in this launch
#define PHMC_STEP 2   // head: it takes a leapfrog step; tail: its trajectory is over
#define PHMC_NAN 4    // head: NaN momentum, no position step (hmc.py:56-57)

// start of a transition (hmc.py:41-48,72 with p = Lm z), first momentum half step and position step (hmc.py:52-58)
template <int NDB>
__global__ __launch_bounds__(256) void k_phmc_head(int D, Chains ch, IterParams ip, PhmcMass pm, double eps) {
  using S = PhmcShape<NDB>;
  constexpr int DP = S::DP, VLD = S::VLD;
  extern __shared__ double phmc_lds[];
  __shared__ int flag[16];
  double* mat = phmc_lds;
  double* vs = mat + S::MAT;
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const int c0 = blockIdx.x * 16;
  int begun = 0, stepping = 0;
  for (int jj = 0; jj < 4; ++jj) {
    const int j = wv + 4 * jj, c = c0 + j;
    double* v = vs + j * VLD;
    int f = 0;
    if (c < ch.n) {
      const int ph = ch.phase[c];
      const long long it = ch.iter[c];
      if (ph == 1) {
        f = PHMC_STEP;
      } else if (ph == 0 && it < ip.iter_limit) {
        const int ns = hmc_begin_dev(D, DP, ch, ip, c, lane, it, v);  // (p' Mass^-1 p / 2 = z'z / 2)
        f = PHMC_BEGUN | (ns > 0 ? PHMC_STEP : 0);
      }
    }
    for (int d = lane; d < DP; d += 64)
      if (!(f & PHMC_BEGUN) || d >= D) v[d] = 0.0;
    if (lane == 0) flag[j] = f;
    begun |= f & PHMC_BEGUN;
    stepping |= f & PHMC_STEP;
  }
  const int any_begun = __syncthreads_or(begun);
  const int any_step = __syncthreads_or(stepping);
  if (!any_begun && !any_step) return;
  if (any_begun) phmc_product<NDB>(pm.Lm, mat, vs, tid);  // p = Lm z
  for (int jj = 0; jj < 4; ++jj) {
    const int j = wv + 4 * jj, c = c0 + j;
    double* v = vs + j * VLD;
    const int f = flag[j];
    if (f & PHMC_STEP) {
      // (a chain that has just begun: its gradient is the current point's, which hmc_copy above has moved to trj as well)
      const double* __restrict__ gr = (f & PHMC_BEGUN) ? ch.cur.grad : ch.trj.grad;
      int isnan_ = 0;
      for (int d = lane; d < D; d += 64) {
        const size_t o = (size_t)c * DP + d;
        const double p0 = (f & PHMC_BEGUN) ? v[d] : ch.p[o];
        const double p = fma(eps * 0.5, gr[o], p0);
        ch.p[o] = p;
        v[d] = p;
        isnan_ |= (p != p);
      }
      const unsigned long long nan = __ballot(isnan_);
      if (nan && lane == 0) {
        ch.status[c] |= 2;
        ch.steps_left[c] = 1;
        flag[j] = f | PHMC_NAN;
      }
    } else if (f & PHMC_BEGUN) {  // a trajectory of zero steps: the momentum is the proposal's
      for (int d = lane; d < D; d += 64) {
        ch.p[(size_t)c * DP + d] = v[d];
        v[d] = 0.0;
      }
    }
  }
  if (!any_step) return;
  phmc_product<NDB>(pm.Minv, mat, vs, tid);  // Mass^-1 p
  for (int jj = 0; jj < 4; ++jj) {
    const int j = wv + 4 * jj, c = c0 + j;
    const double* v = vs + j * VLD;
    const int f = flag[j];
    if ((f & PHMC_STEP) && !(f & PHMC_NAN))
      for (int d = lane; d < D; d += 64) ch.trj.w[(size_t)c * DP + d] = fma(eps, v[d], ch.trj.w[(size_t)c * DP + d]);
  }
}

// gradient / log joint at the new position, second momentum half step (hmc.py:60-62); end of a transition (hmc.py:64-84)
template <int NDB>
__global__ __launch_bounds__(256) void k_phmc_tail(DevData dd, Chains ch, IterParams ip, PhmcMass pm, double eps, int nsplit) {
  using S = PhmcShape<NDB>;
  constexpr int DP = S::DP, VLD = S::VLD;
  extern __shared__ double phmc_lds[];
  __shared__ int flag[16];
  double* mat = phmc_lds;
  double* vs = mat + S::MAT;
  const int D = dd.D;
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const int c0 = blockIdx.x * 16;
  for (int jj = 0; jj < 4; ++jj) {
    const int c = c0 + wv + 4 * jj;
    if (c < ch.n && ch.phase[c] == 1) hmc_finish_eval(dd, ch, c, lane, nsplit);
  }
  __syncthreads();
  int ending = 0;
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
        f = PHMC_STEP;
      }
    }
    for (int d = lane; d < DP; d += 64) v[d] = (f && d < D) ? ch.p[(size_t)c * DP + d] : 0.0;
    if (lane == 0) flag[j] = f;
    ending |= f;
  }
  if (!__syncthreads_or(ending)) return;
  phmc_product<NDB>(pm.Minv, mat, vs, tid);  // Mass^-1 p of the proposals
  for (int jj = 0; jj < 4; ++jj) {
    const int j = wv + 4 * jj, c = c0 + j;
    const double* v = vs + j * VLD;
    if (!flag[j]) continue;
    const long long it = ch.iter[c];
    double kin = 0.0;
    for (int d = lane; d < D; d += 64) { const double pl = ch.p[(size_t)c * DP + d]; kin = fma(pl, v[d], kin); }
    const double Hc = ch.Hcur[c];
    const double Hp = -ch.trj.ljl[c] + 0.5 * wave_sum(kin);  // hmc.py:69
    const double ratio = -Hp + Hc;
    // a chain FAILS (include/rmhmc.h) on a NaN momentum or a Hamiltonian that is not finite at either end: rejected, state untouched
    const bool failed = (ch.status[c] & 2) || !isfinite(Hc) || !isfinite(Hp);
    const bool accept = !failed && mh_accept(ratio, draw_u_acc(ip, c, c, it));  // hmc.py:77
    if (accept) hmc_copy(ch.cur, ch.trj, c, D, DP, lane);
    __builtin_amdgcn_wave_barrier();  // (a lane reads back only what it wrote itself)
    if (failed && lane == 0) ch.status[c] |= 2;
    close_transition(D, DP, ch, ip, c, c, lane, it, Hp, accept);
  }
}
