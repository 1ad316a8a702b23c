// plan.h — everything that decides a shape of a context, and nothing that touches a device: the option table, the shape constants
// the decisions depend on, the argument checks of rmhmc_create (plan_check), the plan itself (make_plan: padding, row splits, the int8
// layout, the stepping path), the launch geometry of the int8 assembly and the variant of the adaptive Metropolis kernel.
// No HIP header: this file compiles as plain C++17 with the host compiler, so a shape's plan can be printed and tested on a machine
// without a GPU (tests/helpers/plan_probe.cpp).  rmhmc_hip.hip allocates what the plan says and launches by it; the kernel headers
// include this file for their constants.
#pragma once
#include "../../include/rmhmc.h"

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

// ---- shape constants (each is used by the kernels of the header named) ---------------------------------------------------------------
#define RM_LD 66            // LDS leading dimension of the per-chain DxD matrix (even: 16-byte aligned rows for ds_read_b128, conflict free)

// fused_small.hip.h
#define FS_D 8
#define FS_WAVES 4
#define FS_PT 104                // doubles of one point record in LDS (w, grad, tr, L, Gi, ljl, hld; padded)

// medium_step.hip.h
#define MS_MAXMP 2048  // rows (padded) whose v and c fit the LDS budget
#define MS_GLD 34      // leading dimension of the G^-1 image

template <int NB>
constexpr int ms_lds_doubles(int Mp) {
  return 64 * RM_LD + 32 * MS_GLD + 4 * (16 * NB) * (16 * NB) + 2 * Mp + 12 * 32 + 4 * 40;
}

// metric_i8.hip.h: chains per tile, and the tile shape (2 x WN waves, wave tile 64 chains x 32 TN pairs) of a slice count
#define I8_BM 128
constexpr int i8_tile_wn(int S) { return S <= 6 ? 4 : 2; }
constexpr int i8_tile_tn(int) { return 1; }

// amh.hip.h: rows of the largest on-chip variant of k_amh (AMH_SWITCH)
#define AMH_MAX_ONCHIP_ROWS (256 * 48)

// ---- options -------------------------------------------------------------------------------------------------------------------------
// Tuning options (include/rmhmc.h: rmhmc_create_opts / rmhmc_set_option).  The library reads no environment variables.
struct Options {
  int64_t graph = 1, sorted = 1, inflight = 32, cdyn = 1, crestore = 1, i8_force_rebase = 0;                 // run time
  int64_t ccache = 1, medium = 1, fused = 1, hmc_traj_maxn = -1, fsplit = 0, nsplit_max = 64, nsplit_waves = -1, i8_tail = -1,   // create time
          i8_delta = 1, i8_delta_inner = 1, i8_zdirect = 3;
};
struct OptionDesc { const char* key; int64_t Options::*slot; bool create_only; int64_t lo, hi; };
inline const OptionDesc kOptions[] = {
    {"graph", &Options::graph, false, 0, 1},
    {"sorted", &Options::sorted, false, 0, 1},
    {"inflight", &Options::inflight, false, 0, 1 << 20},
    {"cdyn", &Options::cdyn, false, 0, 1},
    {"crestore", &Options::crestore, false, 0, 1},
    {"i8_force_rebase", &Options::i8_force_rebase, false, 0, 1},
    {"ccache", &Options::ccache, true, 0, 1},
    {"medium", &Options::medium, true, 0, 1},
    {"fused", &Options::fused, true, 0, 1},
    {"hmc_traj_maxn", &Options::hmc_traj_maxn, true, -1, (int64_t)1 << 40},
    {"fsplit", &Options::fsplit, true, 0, 64},
    {"nsplit_max", &Options::nsplit_max, true, 1, 1 << 20},
    {"nsplit_waves", &Options::nsplit_waves, true, -1, 1 << 20},
    {"i8_tail", &Options::i8_tail, true, -1, 1},
    {"i8_delta", &Options::i8_delta, true, 0, 1},
    {"i8_delta_inner", &Options::i8_delta_inner, true, 0, 1},
    {"i8_zdirect", &Options::i8_zdirect, true, 0, 3},  // mask: bit 0 the 4-slice tiles, bit 1 the 5-slice tiles
};
inline const OptionDesc* find_option(const char* key) {
  if (!key) return nullptr;
  for (const OptionDesc& d : kOptions)
    if (!strcmp(d.key, key)) return &d;
  return nullptr;
}
// Why rmhmc_create_opts (at_create) or rmhmc_set_option refuses a value for the option find_option returned
enum OptionError { OPT_OK, OPT_UNKNOWN, OPT_CREATE_ONLY, OPT_RANGE };
inline OptionError check_option(const OptionDesc* d, int64_t value, bool at_create) {
  if (!d) return OPT_UNKNOWN;
  if (d->create_only && !at_create) return OPT_CREATE_ONLY;
  if (value < d->lo || value > d->hi) return OPT_RANGE;
  return OPT_OK;
}

// ---- argument checks -----------------------------------------------------------------------------------------------------------------
// What rmhmc_create refuses before its first device call: RMHMC_OK, or the error code with its message.
struct PlanCheck { int code; const char* msg; };
inline PlanCheck plan_check(int64_t M, int32_t D, int64_t n_chains, int32_t dtype, uint32_t flags) {
  auto no = [](int code, const char* m) { return PlanCheck{code, m}; };
  if (M <= 0 || D <= 0 || n_chains <= 0) return no(RMHMC_ERR_INVALID, "rmhmc_create: bad shape");
  if (dtype != RMHMC_F64) return no(RMHMC_ERR_UNSUPPORTED, "rmhmc_create: only float64 is built (the reference is float64)");
  if (D > 256) return no(RMHMC_ERR_UNSUPPORTED, "rmhmc_create: D > 256 is not supported (64 < D <= 256 uses the blocked large-D path)");
  if (flags & RMHMC_FLAG_ORACLE_LITERAL) return no(RMHMC_ERR_UNSUPPORTED, "rmhmc_create: the literal variant exists only in the CPU oracle");
  if (M > (int64_t)1 << 30 || n_chains > (int64_t)1 << 30) return no(RMHMC_ERR_UNSUPPORTED, "rmhmc_create: M or n_chains too large");
  // (the row passes of the D <= 64 path address X, the batch's c tiles and its leverages with 32-bit byte offsets from a buffer
  //  descriptor's base: buf_rsrc in kernels.hip.h)
  if (D <= 64 && (M + 63) / 64 * 64 * (int64_t)(16 * ((D + 15) / 16)) * 8 >= (int64_t)1 << 32)
    return no(RMHMC_ERR_UNSUPPORTED, "rmhmc_create: the data matrix of the D <= 64 path must stay below 4 GB");
  return no(RMHMC_OK, "");
}

// ---- the plan ------------------------------------------------------------------------------------------------------------------------
// Every shape of a context, fixed at create (arguments that passed plan_check).  What changes afterwards - whether the certificate of
// rmhmc_set_data lets the int8 path run, a late d_hpart - is state of the context, not of the plan.
struct Plan {
  int64_t M = 0, n = 0;
  int D = 0, DP = 0, NB = 0, Mp = 0, nblk = 0;
  bool big = false;          // large-D path: 64 < D <= 256 (large_d.hip.h)
  int nbk = 1, npairs = 1;   // 64-column blocks and block pairs of the large-D path
  int nsplit = 1;            // row splits of the 16-chains-per-wave passes
  int fsplit = 1;            // fp64 assembly of small batches: row ranges per chain (planes in Gpart)
  int gpart_planes = 0;      // planes of Gpart (0: none): the fp64 row ranges and the int8 k-split pieces share them
  bool hpart_at_create = false;  // the fp64 leverage planes of the large-D path (an int8 context gets them only if the certificate fails)
  // int8 metric path (metric_i8.hip.h), all zero / off unless RMHMC_FLAG_INT8_METRIC was given
  bool i8_requested = false;
  int i8S = 0, i8_nks = 0, i8_bn = 128, i8_chunk = 1;  // i8_chunk: k-stages (of 32) per launch
  int NP = 0, NPp = 0;       // column pairs of the lower triangle, padded to the pair block
  int i8_nkp = 0, i8_NRp = 0;
  int nCp = 0;               // chains padded to the tile
  int ksplit_a = 1, ksplit_l = 1;  // k-split pieces of small batches: assembly (planes in Gpart), leverage pass (planes in Rpart)
  bool tail_acc = false;     // the int32 accumulators of the ragged last pair block exist (k_assemble_i8_tail)
  bool tail_always = false;  // option i8_tail = 1: the tail kernel runs whenever there is a ragged block (-1: when it pays)
  int tail_pieces = 1, tail_blocks = 0;  // k pieces the accumulators have room for; 32-pair blocks of the ragged rest
  bool gbase = false;        // large-D path: a copy of the G a delta assembly adds to
  bool i8_lev_full = false;  // the leverage GEMM sums all S slices whatever the inner-iterate rule says (M < 4 D, see make_plan)
  // the stepping path
  bool fused = false;        // small-problem path: D <= 8 and X fits in LDS (fused_small.hip.h)
  size_t fused_lds = 0;
  bool medium = false;       // one-launch leapfrog step for small batches with 8 < D <= 32 (medium_step.hip.h)
  size_t medium_lds = 0;
  bool hmc_traj = false;     // plain HMC in small batches: one launch per trajectory (k_hmc_traj)
};

inline Plan make_plan(int64_t M, int32_t D, int64_t n_chains, uint32_t flags, const Options& opt) {
  Plan p;
  p.M = M; p.D = D; p.n = n_chains;
  p.NB = (D + 15) / 16; p.DP = 16 * p.NB;
  if (D > 64) {  // large-D path: 64-column blocks, NB = 4 tiles inside a block
    p.big = true;
    p.nbk = (D + 63) / 64;
    p.npairs = p.nbk * (p.nbk + 1) / 2;
    p.DP = 64 * p.nbk;
    p.NB = 4;
  }
  p.Mp = (int)((M + 63) / 64 * 64); p.nblk = p.Mp / 64;
  {  // row splits and partial planes
    // row splits of the 16-chains-per-wave passes (option nsplit_waves).  D <= 64: ~2048 wavefronts per launch = ONE round of two
    // four-wave workgroups per CU - measured against the 6144 of rounds 1-2 (three rounds) on one box, interleaved: 14.73-14.92
    // against 14.99-15.08 ms per step at config 3, +2.7 % steps/s at 4096 chains, +6 % at 2048 and 1024 (fewer partial sums to write and
    // to add up, fewer prologues); the blocked large-D passes keep 6144 (config 5: 472.8 against 475.4 ms per step).
    const long long cgroups = (n_chains + 15) / 16, nb16 = p.Mp / 16;
    const long long target = opt.nsplit_waves > 0 ? opt.nsplit_waves : (p.big ? 6144 : 2048);
    long long ns = (target + cgroups - 1) / cgroups;
    if (ns < 1) ns = 1;
    if (ns > nb16) ns = nb16;
    // ... but no more than 64 splits (option nsplit_max): the consumers sum the partials serially.  (Round 1 kept up to Mp/16 splits for
    // long data sets in small batches, when the one-chain-per-wave assembly dominated those shapes anyway; with the row ranges of
    // k_assemble / k_leverage it is the serial sums that cost: D 64, M 10000, 64 / 128 / 256 chains: 2.44 / 2.28 / 2.52 -> 1.69 / 1.49 /
    // 1.99 ms per step, the int8 path at 128-512 chains 10-30 % less; profiles/r02_fp64_batch_sweep.txt)
    if (ns > opt.nsplit_max) ns = opt.nsplit_max;
    p.nsplit = (int)ns;
    if (!p.big) {
      // fp64 assembly (k_assemble: one chain per wavefront over all M rows): below ~1024 chains the launch has fewer wavefronts than
      // the chip has SIMDs, so the rows are cut until ~2048 wavefronts exist (at least 256 rows per range, at most 16 ranges).
      // D 64, M 10000, 512 chains: the step took longer than with 1024 chains (13.0 vs 7.6 ms, profiles/r01_i8_threshold.txt).
      const long long waves = n_chains;
      long long fs = waves >= 1024 ? 1 : std::min<long long>(16, (2048 + waves - 1) / waves);
      fs = std::min<long long>(fs, std::max(1, p.Mp / 256));
      if (opt.fsplit >= 1) fs = opt.fsplit;
      p.fsplit = (int)fs;
    }
  }
  int i8_slices = (int)((flags >> 12) & 7u);
  if (i8_slices == 0) i8_slices = 6;
  if (i8_slices < 4) i8_slices = 4;
  // int32 accumulators: a weight-g set sums (g+1) K products of two bytes, |.| <= 2^14 each, so one launch covers at most
  // i8_chunk stages of 32 (21845 rows at 6 slices); longer contractions are summed over several launches in fp64.
  if (flags & RMHMC_FLAG_INT8_METRIC) {
    const int S = i8_slices;
    p.i8_chunk = std::max(1, (int)(2147483647.0 / (S * 16384.0)) / 32);
    p.i8_requested = true;
    p.i8S = S;
    p.i8_bn = S <= 6 ? 128 : 64;
    p.i8_nks = (int)((M + 31) / 32);
    p.NP = D * (D + 1) / 2; p.NPp = (p.NP + p.i8_bn - 1) / p.i8_bn * p.i8_bn;
    p.i8_nkp = (p.NP + 31) / 32;
    p.i8_NRp = (p.Mp + p.i8_bn - 1) / p.i8_bn * p.i8_bn;
    p.nCp = (int)((n_chains + I8_BM - 1) / I8_BM * I8_BM);
    p.gbase = p.big && opt.i8_delta && S == 6;
    // Leverages h_n = x_n' G^-1 x_n: G^-1 is cut on a grid relative to its LARGEST entry (k_qsplit).  With fewer than a few rows per
    // column the prior's alpha enters G^-1 at full size while h_n sees the data directions only, so the grid step is amplified by
    // cond(G): measured on an MI355X from the 5 most significant of 6 slices, trace term against the fp64 oracle 3e-11 cond(G) - 4e-11
    // at M = 4.8 D (cond 7), 1e-10 at 2.5 D (18), 1.4e-9 at 1.2 D (400), 1.6e-7 at M = 31 < D = 70 (4400), and momentum after one
    // step 3e-9 there.  Below 4 rows per column the leverage GEMM therefore keeps every slice (7e-10 at cond 4700).  A heuristic on the shape:
    // cond(G) depends on alpha and the data too, and ill-conditioned data with M >= 4 D still gets 5 slices (RMHMC_FLAG_INT8_INNER_FULL).
    p.i8_lev_full = M < 4 * (int64_t)D;
    // small batches: cut the k range so that about 256 workgroups exist (at least 8 stages per piece, at most 16 pieces; only
    // when the whole range fits one overflow-safe launch)
    auto pieces = [&](long long tiles, int stages) {
      long long k = std::min<long long>(16, 256 / std::max<long long>(1, tiles));
      k = std::min<long long>(k, stages / 8);
      if (k < 2 || stages > p.i8_chunk || p.big) return 1;  // (large-D: the identity padding of G lives in Gq itself)
      const int per = (int)((stages + k - 1) / k);
      return (stages + per - 1) / per;
    };
    p.ksplit_a = pieces((long long)(p.nCp / I8_BM) * (p.NPp / p.i8_bn), p.i8_nks);
    p.ksplit_l = pieces((long long)(p.nCp / I8_BM) * (p.i8_NRp / p.i8_bn), p.i8_nkp);
    if (p.ksplit_a == 1 && p.i8_bn == 128 && p.NP % 128 != 0 && opt.i8_tail != 0) {
      p.tail_acc = true;
      p.tail_always = opt.i8_tail == 1;
      p.tail_blocks = (p.NP % 128 + 31) / 32;
      p.tail_pieces = (int)std::max<long long>(1, std::min<long long>(8, 256 / ((long long)(p.nCp / I8_BM) * p.tail_blocks)));
    }
  }
  // planes of the fp64 small-batch assembly (shared with the int8 k-split planes, whichever is larger)
  if (p.fsplit > 1 || p.ksplit_a > 1) p.gpart_planes = std::max(p.fsplit, p.ksplit_a);
  p.hpart_at_create = p.big && !p.i8_requested;
  {  // mid-size problems in small batches: one launch per leapfrog step (option medium = 0 disables it)
    // measured per global step at one chain (tools/bench_single.py): australian (D = 15) 108 us vs 218 us generic, heart (D = 14)
    // 85 vs 154, german (D = 25) 236 vs 386
    p.medium = opt.medium && !p.big && D > FS_D && D <= 32 && p.Mp <= MS_MAXMP && n_chains <= 512;
    if (p.medium) p.medium_lds = sizeof(double) * (p.NB == 1 ? ms_lds_doubles<1>(p.Mp) : ms_lds_doubles<2>(p.Mp));
  }
  {  // plain HMC in small batches: one launch per trajectory (option medium = 0 disables it too)
    // any batch for short data sets (rows in registers; australian, tools/bench_hmc_batch.py: 2048 chains 89 M leapfrog-steps/s vs 39 M
    // generic, 512 chains 59 M vs 9 M; at 8192 chains the generic path has caught up since its row passes run in one round of
    // workgroups - 107 M vs 114 M), small batches otherwise
    long long maxn = p.Mp <= 1024 ? (1ll << 40) : 512;
    if (opt.hmc_traj_maxn >= 0) maxn = opt.hmc_traj_maxn;
    p.hmc_traj = opt.medium && !p.big && D <= 32 && n_chains <= maxn;
  }
  {  // small-problem path eligibility (option fused = 0 disables it)
    const size_t lds = ((size_t)(FS_D + 1 + FS_WAVES) * p.Mp + (size_t)FS_WAVES * FS_PT) * sizeof(double);
    if (opt.fused && D <= FS_D && lds <= 160 * 1024) {
      p.fused = true;
      p.fused_lds = lds;
    }
  }
  return p;
}

// ---- launch geometry of the int8 assembly --------------------------------------------------------------------------------------------
// Tiles of one assembly launch over a batch of nCp (padded) chains with the tile shape WN, TN: chain blocks, pair blocks, and the
// ragged last pair block (D = 64: 2080 pairs = 16 blocks of 128 + 32).  Once the full blocks alone fill the chip, the rest goes to
// k_assemble_i8_tail (bit-identical results, see there).  option i8_tail = 0 / 1: never / whenever there is a ragged block.
// tail_ok: the caller's kernel has a tail variant.
struct I8Geometry {
  int nCB, nPB, nPBfull;   // chain blocks, pair blocks, pair blocks without padding
  bool tail;               // the ragged block runs as tiles of its own
  int npb;                 // pair blocks of the main launch
  unsigned nblk_main;      // its workgroups
  int pb32_0, ntail;       // first 32-pair block of the ragged rest, and how many there are
};
inline I8Geometry i8_geometry(const Plan& p, int nCp, int WN, int TN, bool tail_ok = true) {
  I8Geometry g{};
  g.nCB = nCp / I8_BM; g.nPB = p.NPp / (32 * TN * WN);
  g.nPBfull = p.NP / (32 * TN * WN);
  g.tail = tail_ok && p.tail_acc && g.nPBfull < g.nPB && (p.tail_always || (long long)g.nCB * g.nPBfull >= 256);
  g.npb = g.tail ? g.nPBfull : g.nPB;
  g.nblk_main = (unsigned)((long long)(g.nCB < 8 ? g.nCB : (g.nCB + 7) / 8 * 8) * g.npb);  // (fewer than 8 chain blocks: tiles are dealt round)
  g.pb32_0 = g.nPBfull * TN * WN; g.ntail = (p.NP - g.pb32_0 * 32 + 31) / 32;
  return g;
}
// k pieces of the tail kernel for a k piece of nk stages
inline int i8_tail_pieces(const Plan& p, const I8Geometry& g, int nk) {
  return std::max(1, std::min({p.tail_pieces, nk / 8, (int)(256 / std::max(1, g.nCB * g.ntail))}));
}

// ---- adaptive Metropolis ---------------------------------------------------------------------------------------------------------------
// Block size and rows per thread of k_amh: one wavefront per chain when the batch fills the chip and f fits in 16 registers per lane,
// a 256-thread workgroup otherwise (short latency per proposal for few chains, room for long data sets); R = 0: f is streamed.
struct AmhShape { int nt, rows; };
inline AmhShape amh_shape(int64_t M, int64_t n_chains) {
  const int NT = (M <= 64 * 16 && n_chains >= 1024) ? 64 : 256;
  return {NT, M > AMH_MAX_ONCHIP_ROWS ? 0 : (int)((M + NT - 1) / NT)};
}
