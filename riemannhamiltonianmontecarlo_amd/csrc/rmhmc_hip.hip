// rmhmc_hip.hip — host side of librmhmc_hip.so: the C-ABI of include/rmhmc.h on top of the gfx950
// kernels in kernels.hip.h.  No CPU fallback: every entry point needs a HIP device.
//
// Scheduling: the generalised leapfrog of rmhmc.py:96-163 is a fixed sequence of
// kernels, each over all chains; chains are independent, so transitions are started and finished
// asynchronously (k_iter_begin / k_iter_end act only on chains whose trajectory ended) and every
// chain executes one leapfrog step per "global step" whatever its RandomStep.
#include "../../include/rmhmc.h"
#include "../../include/rmhmc_amh.h"
#include "../../include/rmhmc_iwls.h"
#include "../../include/rmhmc_gibbs.h"
#include "../../include/rmhmc_out.h"
#include "../../include/rmhmc_diag.h"
#include "../../include/rmhmc_phmc.h"
#include "../../include/rmhmc_adapt.h"
#include "../../include/rmhmc_ais.h"
#include "../../include/rmhmc_pred.h"
#include "../../include/rmhmc_smc.h"
#include "../../include/rmhmc_quant.h"
#include "../../include/rmhmc_loo.h"
#include "plan.h"
#include "mass.h"
#include "kernels.hip.h"
#include "fused_small.hip.h"
#include "large_d.hip.h"
#include "metric_i8.hip.h"
#include "medium_step.hip.h"
#include "amh.hip.h"
#include "iwls.hip.h"
#include "gibbs.hip.h"
#include "output.hip.h"
#include "diag.hip.h"
#include "phmc.hip.h"
#include "adapt.hip.h"
#include "ais.hip.h"
#include "pred.hip.h"
#include "smc.hip.h"
#include "quant.hip.h"
#include "loo.hip.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace {

thread_local char g_err[512] = "";  // message of a failed rmhmc_create (no context exists yet); per host thread
// hipFuncAttributeMaxDynamicSharedMemorySize is per (function, device), not per context: always raise it to the hardware
// limit, so that two live contexts of different shapes cannot lower each other's launch limit
constexpr int MAX_LDS = 160 * 1024;

struct EvPair { hipEvent_t a, b; };

// The batch of chains a launch works on, with the per-chain arrays and the scratch sized for it.  There is one per context
// (the whole batch); the work-sorted sampler narrows a copy of it to the prefix of chains still running (launch_global_step_prefix).
// How the work is cut up (row splits, row ranges, k pieces) is decided once for the context: the Plan (plan.h).
// (Cutting the batch into 2-4 groups ping-ponged over two streams was measured twice without gain on MI355X - the co-running
// light kernels are starved and the heavy ones slow down by the same total, profiles/r01_groups_sweep.txt.)
struct Group {
  Chains ch{};
  int n = 0;
  int nCp = 0;           // int8 metric path: n padded to the tile
  int8_t* Vs = nullptr;  // int8 metric path: slices of v, [S][nks][nCp][32]
  int8_t* Qs = nullptr;  // slices of the doubled G^-1 entries, [S][nkp][nCp][32]
  double* qscale = nullptr;
  double *Gpart = nullptr, *Rpart = nullptr;  // planes of small batches ([gpart_planes][n][DP*DP], [ksplit_l][n][Mp])
  int* Tq = nullptr;      // int32 accumulators of the ragged last pair block, [pieces][S][nCp][32 ntail] (k_assemble_i8_tail)
  int* vbad = nullptr;
  int* vexp = nullptr;   // per-chain extra binary digits of the v grid (VSlice)
  int* vexp_d = nullptr; int* rebase = nullptr; unsigned long long* dmax = nullptr;  // delta assembly (VSlice / I8Delta)
  unsigned long long* dcount = nullptr;  // [6] delta assemblies by slice count (I8Delta::count, rmhmc_kernel_time "i8_delta_*"; zeroed by chains_init)
  double* Gbase = nullptr;  // large-D path: copy of the G a delta assembly adds to (Gq is factored in place)
  d4* ctile = nullptr;   // c = v(1-2p) of trj.w in the tile layout of k_mompass, [ceil(n/16)][Mp/16][64] x 4 doubles
};

// What one call asks of the stepping code.  The entry point builds it from its own arguments and hands it down by const&; nothing
// below writes it, and the context keeps none of it (rmhmc_ctx::chains is the one exception).  A parameter the call's sampler
// never reads is 0 (K of plain HMC, L of rmhmc_leapfrog, seed and chain_offset where the randomness is the caller's).
// rmhmc.py / hmc.py / HMC with the context's mass matrix (phmc.hip.h) / the same on the tempered target (ais.hip.h): selects the global step
enum Sampler { RMHMC, HMC, PHMC, TPHMC };
struct Run {
  Sampler sampler;
  int L, K;
  double eps;
  uint64_t seed; int64_t chain_offset;  // Philox key of chain c: (seed, chain_offset + c)
  const int* orig;  // work-sorted layout (sample_core): [n] position -> chain index in the caller's order, or nullptr: position = chain
  double beta = 1.0;  // TPHMC only: the temperature (include/rmhmc_ais.h)
};
struct IterBase {  // ... and of the transition bookkeeping of the steps it issues
  long long limit, burn_in, S;
  double* samples;
  bool explicit_rng;
  bool count_done;
};

}  // namespace

// The context IS its plan (plan.h: M, D, n, the padded sizes, the splits, the int8 layout, the stepping path - fixed at create),
// plus the device state and what changes after create.
struct rmhmc_ctx : Plan {
  int device = 0;
  uint32_t flags = 0;
  double alpha = 100.0;
  hipStream_t stream = nullptr;
  Options opt{};
  std::vector<hipEvent_t> flow;  // flow control (option inflight): events recorded every few global steps, see flow_tick
  long long flow_steps = 0, flow_ticks = 0;
  int* stale_list_alloc = nullptr;  // list of the chains that have just rejected a proposal (k_crestore; in use when cdyn and crestore are on)
  DevData dd{};
  Group batch;  // all n chains; batch.ch holds the per-chain arrays
  std::vector<void*> allocs;
  bool have_data = false, chains_ready = false;
  Run chains{};  // stateful API only: written by rmhmc_chains_init, read by rmhmc_chains_run while chains_ready holds
  double *d_Wd = nullptr, *d_hpart = nullptr, *d_Gcopy = nullptr;
  // (options crestore / cdyn / ccache: c = v(1-2p) kept per position in the momentum pass's tile layout; the first pass of a step re-uses
  //  the tiles of chains that did not just reject; those of the chains that did are recomputed by k_crestore, 16 to a wavefront)
  // int8 metric path (metric_i8.hip.h)
  bool i8 = false;           // in use: requested at create (Plan::i8_requested) and not switched off by the set_data certificate
  int i8_inner_drop = 1;     // inner assemblies from S-1 slices (launch_assemble; RMHMC_FLAG_INT8_INNER_FULL: off)
  // (options i8_delta / i8_delta_inner: G at the end of a leapfrog step, and the second position iterate, as the previous iterate's G + the
  //  assembly of the v differences; i8_force_rebase: tests treat every chain as if its v exponent had changed; i8_tail: ragged last pair
  //  block as tiles of its own: -1 when it pays (launch_assemble_i8_t), 0 never, 1 always; i8_zdirect: the 4-slice (bit 0) and 5-slice (bit 1)
  //  tiles in their ZDIRECT form, chosen at launch - both forms are built)
  int8_t* d_Zs = nullptr;
  int* d_ze = nullptr;
  int8_t* d_Zt = nullptr;   // leverage pass: x_a x_b sliced per data row, [S][nkp][NRp][32]
  int* d_zre = nullptr;
  double *d_cmin = nullptr, *d_cmax = nullptr;  // min_n |x_nd|, max_n |x_nd| per column (VSlice)
  double* d_zscale = nullptr;
  I8Pairs pairs{};
  double i8_bound = 0.0;       // certificate of the last set_data (metric_i8.hip.h: "Error bound"), 0 when the path is not requested
  // fixed-metric HMC (phmc.hip.h): the images of rmhmc_phmc_set_mass, [DP][DP] each, allocated by its first call
  double *d_massL = nullptr, *d_massInv = nullptr;
  bool have_mass = false;
  // tempered fixed-metric HMC and annealed importance sampling (ais.hip.h), [n] each, allocated by the first call that needs them:
  // loglik of every chain's current point, that of the last initial evaluation, the log weights of rmhmc_ais_run
  double *d_ais_ll = nullptr, *d_ais_ll0 = nullptr, *d_ais_logw = nullptr;
  // unit-API staging (device)
  double *d_z = nullptr, *d_ulen = nullptr, *d_gdir = nullptr, *d_uacc = nullptr;
  int *d_nsteps = nullptr, *d_dir = nullptr, *d_done = nullptr;
  long long* d_steps0 = nullptr;
  unsigned long long* d_miniter = nullptr;
  // work-sorted layout of the bulk sampler (sample_core)
  int* d_orig = nullptr;            // [n] position -> chain index in the caller's order (Run::orig of a sorted run)
  long long* d_T = nullptr;         // [2n] scratch: trajectory-length sums / counters back in the caller's order
  // progress reports of the bulk samplers (rmhmc_set_progress)
  rmhmc_progress_fn progress_fn = nullptr;
  void* progress_user = nullptr;
  long long progress_first = 0, progress_every = 0;
  // timing
  double write_out_seconds = 0.0;  // host wall time of the last write_out (rmhmc_kernel_time "write_out", include/rmhmc_out.h)
  bool timing = false;
  std::map<std::string, std::vector<EvPair>> events;
  std::vector<EvPair> pool;
  char err[512] = "";
};

namespace {

int fail(rmhmc_ctx* ctx, int code, const std::string& msg) {
  snprintf(ctx ? ctx->err : g_err, 512, "%s", msg.c_str());
  return code;
}

#define HIPCK(call)                                                                                        \
  do {                                                                                                     \
    hipError_t e_ = (call);                                                                                \
    if (e_ != hipSuccess)                                                                                  \
      return fail(ctx, RMHMC_ERR_RUNTIME, std::string(hipGetErrorString(e_)) + " in " #call " (" __FILE__ ":" + std::to_string(__LINE__) + ")"); \
  } while (0)

template <typename T>
int dalloc(rmhmc_ctx* ctx, T** p, size_t count) {
  void* q = nullptr;
  size_t bytes = (count ? count : 1) * sizeof(T);
  HIPCK(hipMalloc(&q, bytes));
  HIPCK(hipMemsetAsync(q, 0, bytes, ctx->stream));
  ctx->allocs.push_back(q);
  *p = (T*)q;
  return RMHMC_OK;
}

// The device memory of one call (dalloc's lives as long as the context): every buffer it hands out is freed when it goes out of
// scope, on every path.  Freeing is all it does: the function that declares it leaves the stream idle before it returns successfully.
struct CallMem {
  rmhmc_ctx* ctx;
  std::vector<void*> held;
  explicit CallMem(rmhmc_ctx* c) : ctx(c) {}
  CallMem(const CallMem&) = delete;
  CallMem& operator=(const CallMem&) = delete;
  ~CallMem() { for (void* q : held) (void)hipFree(q); }
  template <typename T>
  int alloc(T** p, size_t bytes) {  // (uninitialised, unlike dalloc's)
    void* q = nullptr;
    HIPCK(hipMalloc(&q, bytes));
    held.push_back(q);
    *p = (T*)q;
    return RMHMC_OK;
  }
};

// hipFuncAttributeMaxDynamicSharedMemorySize of one kernel (MAX_LDS above: per function and device, so never lowered)
template <typename K>
int raise_lds(rmhmc_ctx* ctx, K kernel, int bytes) {
  HIPCK(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  return RMHMC_OK;
}

struct Timed {
  rmhmc_ctx* ctx;
  hipStream_t st;
  EvPair ev{};
  bool on;
  Timed(rmhmc_ctx* c, const char* name, hipStream_t s) : ctx(c), st(s), on(c->timing) {
    if (!on) return;
    if (!ctx->pool.empty()) { ev = ctx->pool.back(); ctx->pool.pop_back(); }
    else { (void)hipEventCreate(&ev.a); (void)hipEventCreate(&ev.b); }
    (void)hipEventRecord(ev.a, st);
    ctx->events[name].push_back(ev);
  }
  ~Timed() { if (on) (void)hipEventRecord(ev.b, st); }
};

// Launch one kernel (or a short run of them).  fn(stream) enqueues it; name keys the optional event timing.
template <typename F>
void launch(rmhmc_ctx* ctx, const char* name, F&& fn) {
  Timed t(ctx, name, ctx->stream);
  fn(ctx->stream);
}

// Flow control (option inflight): the host is never more than `inflight` global steps ahead of the device.  Every inflight/4 steps an
// event goes into the stream, and before the host records the fifth it waits for the first.  A run of several hundred steps used to be
// queued in one go (~45 dispatches per step: tens of thousands of AQL packets), which costs nothing on the bare runtime but is what an
// intercepting tool's proxy queue cannot take ("Profiler note"); a bounded queue is the better citizen anyway.
void flow_tick(rmhmc_ctx* ctx, long long steps = 1) {
  const long long w = ctx->opt.inflight;
  if (w <= 0) return;
  ctx->flow_steps += steps;
  const long long stride = std::max<long long>(1, w / 4);
  if (ctx->flow_steps < stride) return;
  ctx->flow_steps = 0;
  if (ctx->flow.empty()) return;  // (created by rmhmc_create_opts)
  hipEvent_t e = ctx->flow[ctx->flow_ticks % 4];
  if (ctx->flow_ticks >= 4) (void)hipEventSynchronize(e);
  (void)hipEventRecord(e, ctx->stream);
  ctx->flow_ticks++;
}

#define NB_SWITCH(ctx, ...)                                               \
  switch ((ctx)->NB) {                                                    \
    case 1: { constexpr int NB_ = 1; __VA_ARGS__; } break;                \
    case 2: { constexpr int NB_ = 2; __VA_ARGS__; } break;                \
    case 3: { constexpr int NB_ = 3; __VA_ARGS__; } break;                \
    default: { constexpr int NB_ = 4; __VA_ARGS__; } break;               \
  }

// the steps of four columns of a DrawProduct (pred_ksteps, loo's ksteps)
static_assert(PRED_MAX_D == 256 && LOO_MAX_D == 256, "the cases of KS_SWITCH end at 64 steps");
#define KS_SWITCH(ksteps, ...)                                            \
  switch (ksteps) {                                                       \
    case 4: { constexpr int KS_ = 4; __VA_ARGS__; } break;                \
    case 8: { constexpr int KS_ = 8; __VA_ARGS__; } break;                \
    case 16: { constexpr int KS_ = 16; __VA_ARGS__; } break;              \
    case 24: { constexpr int KS_ = 24; __VA_ARGS__; } break;              \
    case 32: { constexpr int KS_ = 32; __VA_ARGS__; } break;              \
    case 40: { constexpr int KS_ = 40; __VA_ARGS__; } break;              \
    case 48: { constexpr int KS_ = 48; __VA_ARGS__; } break;              \
    case 56: { constexpr int KS_ = 56; __VA_ARGS__; } break;              \
    default: { constexpr int KS_ = 64; __VA_ARGS__; } break;              \
  }

// the tile widths of diag_tile_width and quant_tile_width; `otherwise` runs for any other
#define TW_SWITCH(tw, otherwise, ...)                                     \
  switch (tw) {                                                           \
    case 1: { constexpr int TW_ = 1; __VA_ARGS__; } break;                \
    case 2: { constexpr int TW_ = 2; __VA_ARGS__; } break;                \
    case 4: { constexpr int TW_ = 4; __VA_ARGS__; } break;                \
    case 8: { constexpr int TW_ = 8; __VA_ARGS__; } break;                \
    case 16: { constexpr int TW_ = 16; __VA_ARGS__; } break;              \
    case 32: { constexpr int TW_ = 32; __VA_ARGS__; } break;              \
    case 64: { constexpr int TW_ = 64; __VA_ARGS__; } break;              \
    default: { otherwise; } break;                                        \
  }

#define I8_SWITCH(ctx, ...) I8_SWITCH_S((ctx)->i8S, __VA_ARGS__)
#define I8_SWITCH_S(sval, ...)                                                                       \
  switch (sval) {                                                                                    \
    case 4: { constexpr int S_ = 4, WN_ = i8_tile_wn(4), TN_ = i8_tile_tn(4); __VA_ARGS__; } break;  \
    case 5: { constexpr int S_ = 5, WN_ = i8_tile_wn(5), TN_ = i8_tile_tn(5); __VA_ARGS__; } break;  \
    case 6: { constexpr int S_ = 6, WN_ = i8_tile_wn(6), TN_ = i8_tile_tn(6); __VA_ARGS__; } break;  \
    default: { constexpr int S_ = 7, WN_ = i8_tile_wn(7), TN_ = i8_tile_tn(7); __VA_ARGS__; } break; \
  }

// Delta assembly of the evaluation that ends a leapfrog step (I8Delta in metric_i8.hip.h): the last position iterate has left its N in
// the slice planes and its G - summed from all six slices - in Gq, and v moves by 1e-6 between the two points, so the difference
// needs four slices (10 slice products) where the full assembly needs six (21).
static bool use_delta(const rmhmc_ctx* ctx, const Run& run, const Group& g) {
  return ctx->i8 && ctx->opt.i8_delta && (!ctx->big || g.Gbase) && ctx->i8S == 6 && g.ctile && ctx->ksplit_a <= 1 && run.K >= 2 && g.dmax;
}
// The second position iterate as a delta of the first (both inner iterates on five slices: it = 2 < K - 1; later inner iterates would need
// the N of a predecessor whose planes hold differences)
static bool use_delta_inner(const rmhmc_ctx* ctx, const Run& run, const Group& g, int it) {
  return use_delta(ctx, run, g) && ctx->opt.i8_delta_inner && ctx->i8_inner_drop && it == 2 && it < run.K - 1;
}
template <int MODE>
void launch_rowpass(rmhmc_ctx* ctx, Group& g, const double* w, double* out0, double* out2 = nullptr, bool delta = false) {
  launch(ctx, "rowpass", [&](hipStream_t st) {
    if (ctx->big) {
      dim3 grid((unsigned)((g.n + 15) / 16), ctx->nsplit);
      hipLaunchKernelGGL((k_rowpass_big<MODE>), grid, dim3(256), 0, st, ctx->dd, g.n, ctx->nsplit, ctx->nbk, g.ch.phase, w, out0, out2,
                         g.ch.gpart, g.ch.ljl_part, g.ctile);
      return;
    }
    dim3 grid((unsigned)((g.n + 63) / 64), ctx->nsplit);
    if (ctx->i8 && MODE != RP_G) {  // int8 metric path: v goes out as byte slices (no fp64 row vector, no k_vsplit)
      // (vbad and dmax are clear: the factor kernel behind the previous assembly has reset them, Chains::i8_vbad / i8_dmax)
      const VSlice vs{g.Vs, g.vbad, ctx->i8_nks, g.nCp, ctx->i8S, g.vexp, ctx->d_cmin, ctx->d_cmax};
      // (with c tiles nobody reads a natural-layout c on this path: k_mompass and k_trvec take the tiles)
      if (MODE != RP_G && delta) {
        VSlice vd = vs;
        vd.vexp_d = g.vexp_d; vd.rebase = g.rebase; vd.dmax = g.dmax; vd.force_rebase = (int)ctx->opt.i8_force_rebase;
        if (MODE == RP_F) {
          NB_SWITCH(ctx, hipLaunchKernelGGL((k_rowpass<NB_, RP_F, 6, false, true>), grid, dim3(256), 0, st, ctx->dd, g.n, ctx->nsplit, g.ch.phase, w,
                                            out0, nullptr, g.ch.gpart, g.ch.ljl_part, vd, g.ctile, g.ch.cstale));
        } else {
          NB_SWITCH(ctx, hipLaunchKernelGGL((k_rowpass<NB_, RP_V, 6, true, true>), grid, dim3(256), 0, st, ctx->dd, g.n, ctx->nsplit, g.ch.phase, w,
                                            out0, out2, g.ch.gpart, g.ch.ljl_part, vd, g.ctile, g.ch.cstale));
        }
      } else if (g.ctile && MODE == RP_F) {
        I8_SWITCH(ctx, NB_SWITCH(ctx, hipLaunchKernelGGL((k_rowpass<NB_, MODE, S_, false>), grid, dim3(256), 0, st, ctx->dd, g.n, ctx->nsplit, g.ch.phase, w,
                                                        out0, nullptr, g.ch.gpart, g.ch.ljl_part, vs, g.ctile, g.ch.cstale)));
      } else {
        I8_SWITCH(ctx, NB_SWITCH(ctx, hipLaunchKernelGGL((k_rowpass<NB_, MODE, S_>), grid, dim3(256), 0, st, ctx->dd, g.n, ctx->nsplit, g.ch.phase, w, out0,
                                                        out2, g.ch.gpart, g.ch.ljl_part, vs, g.ctile, g.ch.cstale)));
      }
      return;
    }
    NB_SWITCH(ctx, hipLaunchKernelGGL((k_rowpass<NB_, MODE>), grid, dim3(256), 0, st, ctx->dd, g.n, ctx->nsplit, g.ch.phase, w, out0,
                                      out2, g.ch.gpart, g.ch.ljl_part, VSlice{}, g.ctile, g.ch.cstale));
  });
}

// int8 metric path: cut v into slices, then the sliced GEMM against the fixed slices of x_a x_b (metric_i8.hip.h)
template <int S, int WN, int TN>
void launch_assemble_i8_t(rmhmc_ctx* ctx, Group& g, const double* v, hipStream_t st, int part, bool delta = false, int seff = 6, int need_lo = 0,
                          int need_hi = 0) {
  // delta: this instantiation on the V planes seff - S .. seff - 1 (seff = 6: all digits count; 5: an inner iterate), added to Gq if the
  // digits *dmax asks for lie in [need_lo, need_hi] (I8Delta)
  const size_t vplane = (size_t)ctx->i8_nks * g.nCp * 32;
  const int8_t* const Vs = g.Vs + (delta ? (size_t)(seff - S) * vplane : 0);
  const I8Delta dl{delta ? g.dmax : nullptr, delta ? g.rebase : nullptr, delta ? std::ldexp(1.0, -8 * (seff - S)) : 1.0, need_lo, need_hi,
                   (delta && ctx->big) ? g.Gbase : nullptr};
  const int* const vexp = delta ? g.vexp_d : g.vexp;
  const int acc0 = delta ? 2 : 0;
  if (part == 0) {
    if (delta) {  // (large-D path: the planes hold N of the previous iterate, they get the digits of the difference)
      (void)hipMemsetAsync(g.dmax, 0, sizeof(unsigned long long), st);
      hipLaunchKernelGGL((k_vsplit<S, true>), dim3((unsigned)((g.n + 7) / 8)), dim3(256), 0, st, v, ctx->Mp, g.n, g.ch.phase, ctx->i8_nks, g.nCp, g.Vs,
                         g.vbad, ctx->D, ctx->DP, ctx->dd.inv_alpha, g.ch.Gq, g.vexp, VDelta{g.vexp_d, g.rebase, g.dmax, (int)ctx->opt.i8_force_rebase});
      return;
    }
    hipLaunchKernelGGL((k_vsplit<S>), dim3((unsigned)((g.n + 7) / 8)), dim3(256), 0, st, v, ctx->Mp, g.n, g.ch.phase, ctx->i8_nks, g.nCp, g.Vs, g.vbad,
                       ctx->D, ctx->DP, ctx->dd.inv_alpha, g.ch.Gq, g.vexp, VDelta{});
    return;
  }
  const I8Geometry t = i8_geometry(*ctx, g.nCp, WN, TN, WN == 4);  // (k_assemble_i8_tail pairs with the 8-wave tile)
  // option i8_zdirect: the ZDIRECT form of the tile where there is one (S = 4, 5: one bit of the option each); both forms are in the
  // library, and each launches with the LDS size of its own instantiation
  auto main_tiles = [&](dim3 grid, auto... args) {
    if (i8_zdirect_tile(S, WN, TN) && i8_zdirect_on(ctx->opt.i8_zdirect, S))
      hipLaunchKernelGGL((k_assemble_i8<S, WN, TN, true>), grid, dim3(128 * WN), (i8_lds_bytes<S, WN, TN, true>()), st, args...);
    else
      hipLaunchKernelGGL((k_assemble_i8<S, WN, TN>), grid, dim3(128 * WN), (i8_lds_bytes<S, WN, TN>()), st, args...);
  };
  if (ctx->ksplit_a > 1) {  // small batch: too few tiles to fill the chip, so the k range is cut into planes that are summed afterwards
    // (a plan with k pieces has no tail accumulators: the main tiles are all pair blocks)
    const size_t plane = (size_t)g.n * ctx->DP * ctx->DP;
    main_tiles(dim3(t.nblk_main, (unsigned)ctx->ksplit_a), (const int8_t*)g.Vs, (const int8_t*)ctx->d_Zs, g.nCp, ctx->i8_nks,
               0, ctx->i8_nks, 0, ctx->pairs, g.n, (const int*)g.ch.phase, (const int*)g.vbad, ctx->DP, ctx->dd.inv_alpha, g.Gpart, plane, (const int*)g.vexp, t.npb,
               I8Delta{nullptr, nullptr, 1.0, 0, 0, nullptr});
    hipLaunchKernelGGL(k_sum_planes, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, st, g.ch.Gq, g.Gpart, ctx->ksplit_a, plane, plane);
    return;
  }
  // the k range in pieces whose int32 sums cannot overflow whatever the data (one piece up to M = 21845 at 6 slices)
  for (int ks0 = 0; ks0 < ctx->i8_nks; ks0 += ctx->i8_chunk) {
    const int nk = std::min(ctx->i8_chunk, ctx->i8_nks - ks0);
    if (t.nblk_main)
      main_tiles(dim3(t.nblk_main), Vs, (const int8_t*)ctx->d_Zs, g.nCp, ctx->i8_nks, ks0, nk, (ks0 > 0 ? 1 : 0) | acc0, ctx->pairs, g.n,
                 (const int*)g.ch.phase, (const int*)g.vbad, ctx->DP, ctx->dd.inv_alpha, g.ch.Gq, (size_t)0, vexp, t.npb, dl);
    if (t.tail) {
      const int pieces = i8_tail_pieces(*ctx, t, nk);
      hipLaunchKernelGGL((k_assemble_i8_tail<S>), dim3((unsigned)(t.nCB * t.ntail), (unsigned)pieces), dim3(128), (i8_lds_bytes<S, 1, 1>()), st, Vs, ctx->d_Zs,
                         g.nCp, ctx->pairs.NPp, ctx->pairs.NP, ctx->i8_nks, ks0, nk, g.n, t.pb32_0, t.ntail, g.Tq, dl);
      hipLaunchKernelGGL((k_assemble_i8_tailsum<S>), dim3((unsigned)(((size_t)g.n * 32 * t.ntail + 255) / 256)), dim3(256), 0, st, g.Tq, pieces, g.nCp, t.ntail,
                         t.pb32_0, (ks0 > 0 ? 1 : 0) | acc0, ctx->pairs, g.n, g.ch.phase, g.vbad, ctx->DP, ctx->dd.inv_alpha, g.ch.Gq, vexp, dl);
    }
  }
}
// Delta assembly (use_delta: S = 6, the 8-wave tile, no k-split planes): one launch each of the main tiles, the ragged pair block's tiles and their
// sum; the kernels pick the slice count the difference needs from *dmax themselves (k_assemble_i8_sel).  seff 6: full accuracy; 5: inner iterate
void launch_assemble_i8_delta(rmhmc_ctx* ctx, Group& g, hipStream_t st, int seff) {
  constexpr int WN = 4, TN = 1;
  const size_t vplane = (size_t)ctx->i8_nks * g.nCp * 32;
  const I8Delta dl{g.dmax, g.rebase, 1.0, 0, 0, ctx->big ? g.Gbase : nullptr};
  const I8Geometry t = i8_geometry(*ctx, g.nCp, WN, TN);
  constexpr int lds = i8_lds_bytes<6, WN, TN>() > i8_lds_bytes<4, WN, TN>() ? i8_lds_bytes<6, WN, TN>() : i8_lds_bytes<4, WN, TN>();
  static_assert(lds >= (i8_lds_bytes<5, WN, TN>()), "dynamic LDS of the widest instantiation");
  constexpr int lds_t = i8_lds_bytes<6, 1, 1>() > i8_lds_bytes<4, 1, 1>() ? i8_lds_bytes<6, 1, 1>() : i8_lds_bytes<4, 1, 1>();
  static_assert(lds_t >= (i8_lds_bytes<5, 1, 1>()), "dynamic LDS of the widest tail instantiation");
  // the assembly is counted once (g.dcount): by the first k piece's main launch, or by its tail launch when there are no main tiles
  I8Delta dlc = dl;
  dlc.count = g.dcount;
  // option i8_zdirect picks the kernel whose S' = 4 (bit 0) and S' = 5 (bit 1) branches are the ZDIRECT form; the 6-slice branch is the
  // same code in all four.  lds: the 6-slice LDS form, wider than either ZDIRECT form
  static_assert(lds >= (i8_lds_bytes<5, WN, TN, true>()) && lds >= (i8_lds_bytes<4, WN, TN, true>()), "dynamic LDS of the widest instantiation");
  auto main_tiles = [&](dim3 grid, auto... args) {
    switch ((int)ctx->opt.i8_zdirect) {
      case 3: hipLaunchKernelGGL((k_assemble_i8_sel<WN, TN, 3>), grid, dim3(128 * WN), lds, st, args...); break;
      case 2: hipLaunchKernelGGL((k_assemble_i8_sel<WN, TN, 2>), grid, dim3(128 * WN), lds, st, args...); break;
      case 1: hipLaunchKernelGGL((k_assemble_i8_sel<WN, TN, 1>), grid, dim3(128 * WN), lds, st, args...); break;
      default: hipLaunchKernelGGL((k_assemble_i8_sel<WN, TN, 0>), grid, dim3(128 * WN), lds, st, args...);
    }
  };
  for (int ks0 = 0; ks0 < ctx->i8_nks; ks0 += ctx->i8_chunk) {
    const int nk = std::min(ctx->i8_chunk, ctx->i8_nks - ks0);
    if (t.nblk_main)
      main_tiles(dim3(t.nblk_main), (const int8_t*)g.Vs, vplane, seff, (const int8_t*)ctx->d_Zs, g.nCp, ctx->i8_nks, ks0, nk, (ks0 > 0 ? 1 : 0) | 2, ctx->pairs,
                 g.n, (const int*)g.ch.phase, (const int*)g.vbad, ctx->DP, ctx->dd.inv_alpha, g.ch.Gq, (size_t)0, (const int*)g.vexp_d, t.npb,
                 ks0 == 0 ? dlc : dl);
    if (t.tail) {
      const int pieces = i8_tail_pieces(*ctx, t, nk);
      hipLaunchKernelGGL(k_assemble_i8_tail_sel, dim3((unsigned)(t.nCB * t.ntail), (unsigned)pieces), dim3(128), lds_t, st, g.Vs, vplane, seff, ctx->d_Zs,
                         g.nCp, ctx->pairs.NPp, ctx->pairs.NP, ctx->i8_nks, ks0, nk, g.n, t.pb32_0, t.ntail, g.Tq, (ks0 == 0 && !t.nblk_main) ? dlc : dl);
      hipLaunchKernelGGL(k_assemble_i8_tailsum_sel, dim3((unsigned)(((size_t)g.n * 32 * t.ntail + 255) / 256)), dim3(256), 0, st, seff, g.Tq, pieces, g.nCp, t.ntail,
                         t.pb32_0, (ks0 > 0 ? 1 : 0) | 2, ctx->pairs, g.n, g.ch.phase, g.vbad, ctx->DP, ctx->dd.inv_alpha, g.ch.Gq, g.vexp_d, dl);
    }
  }
}
// leverage pass of the int8 path: part 0 cuts G^-1 into slices, part 1 is the GEMM (R = c .* h into rv0, v is dead by then)
template <int S, int WN, int TN>
void launch_leverage_i8_t(rmhmc_ctx* ctx, Group& g, hipStream_t st, int part) {
  if (part == 0) {
    hipLaunchKernelGGL((k_qsplit<S>), dim3((unsigned)g.n), dim3(256), 0, st, g.ch.trj.Ginv, ctx->DP, ctx->pairs, g.ch.phase, ctx->i8_nkp, g.nCp,
                       g.Qs, g.qscale);
    return;
  }
  const int nCB = g.nCp / I8_BM, nRB = ctx->i8_NRp / (32 * TN * WN);
  const unsigned nblk = (unsigned)(nCB < 8 ? nCB * nRB : (nCB + 7) / 8 * 8 * nRB);
  auto tiles = [&](dim3 grid, auto... args) {  // (option i8_zdirect, as in launch_assemble_i8_t)
    if (i8_zdirect_tile(S, WN, TN) && i8_zdirect_on(ctx->opt.i8_zdirect, S))
      hipLaunchKernelGGL((k_leverage_i8<S, WN, TN, true>), grid, dim3(128 * WN), (i8_lds_bytes<S, WN, TN, true>()), st, args...);
    else
      hipLaunchKernelGGL((k_leverage_i8<S, WN, TN>), grid, dim3(128 * WN), (i8_lds_bytes<S, WN, TN>()), st, args...);
  };
  if (ctx->ksplit_l > 1) {
    const size_t plane = (size_t)g.n * ctx->Mp;
    tiles(dim3(nblk, (unsigned)ctx->ksplit_l), (const int8_t*)g.Qs, (const int8_t*)ctx->d_Zt, g.nCp, ctx->i8_NRp, ctx->i8_nkp, 0, ctx->i8_nkp, 0,
          (ctx->big || g.ctile) ? 0 : 1, g.n, ctx->Mp, (const int*)g.ch.phase, (const double*)g.qscale, (const double*)ctx->d_zscale,
          (const double*)g.ch.rv2, g.Rpart, plane);
    hipLaunchKernelGGL(k_sum_planes, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, st, g.ch.rv0, g.Rpart, ctx->ksplit_l, plane, plane);
    return;
  }
  for (int kp0 = 0; kp0 < ctx->i8_nkp; kp0 += ctx->i8_chunk) {
    const int nk = std::min(ctx->i8_chunk, ctx->i8_nkp - kp0);
    tiles(dim3(nblk), (const int8_t*)g.Qs, (const int8_t*)ctx->d_Zt, g.nCp, ctx->i8_NRp, ctx->i8_nkp, kp0, nk, kp0 > 0 ? 1 : 0,
          (ctx->big || g.ctile) ? 0 : 1, g.n, ctx->Mp, (const int*)g.ch.phase, (const double*)g.qscale, (const double*)ctx->d_zscale,
          (const double*)g.ch.rv2, g.ch.rv0, (size_t)0);
  }
}
// inner: an assembly whose G only steers a fixed-point iterate (the position iterations before the last, rmhmc.py:116-122).  With
// ctx->i8_inner_drop it is summed from the S-1 most significant slices of the same operands (balanced digits: dropping the last digit
// IS rounding to the coarser grid), 15 slice products instead of 21.
// keep_base (large-D path): this G is the base of a delta assembly to come; Gq will be factored in place, so a copy is kept
void launch_assemble(rmhmc_ctx* ctx, Group& g, const double* v, bool inner = false, bool delta = false, bool keep_base = false) {
  if (ctx->i8 && delta && ctx->big)
    launch(ctx, "vsplit", [&](hipStream_t st) { launch_assemble_i8_t<6, 4, 1>(ctx, g, v, st, 0, true); });
  if (ctx->i8 && delta && inner) {  // (use_delta_inner: five-slice accuracy)
    launch(ctx, "assemble_i8_inner_delta", [&](hipStream_t st) { launch_assemble_i8_delta(ctx, g, st, 5); });
    return;
  }
  if (ctx->i8 && delta) {  // (use_delta: S = 6, WN = 4)
    launch(ctx, "assemble_i8_delta", [&](hipStream_t st) { launch_assemble_i8_delta(ctx, g, st, 6); });
    return;
  }
  if (ctx->i8) {
    if (ctx->big)  // (the generic row pass already wrote the slices)
      launch(ctx, "vsplit", [&](hipStream_t st) { I8_SWITCH(ctx, (launch_assemble_i8_t<S_, WN_, TN_>(ctx, g, v, st, 0))); });
    const int suse = (inner && ctx->i8_inner_drop && ctx->i8S == 6) ? 5 : ctx->i8S;  // (5 -> 4 costs parity: 2e-9 on theta at M = 97)
    launch(ctx, suse == ctx->i8S ? "assemble_i8" : "assemble_i8_inner", [&](hipStream_t st) {
      I8_SWITCH_S(suse, (launch_assemble_i8_t<S_, WN_, TN_>(ctx, g, v, st, 1)));
      if (keep_base && ctx->big && g.Gbase)
        (void)hipMemcpyAsync(g.Gbase, g.ch.Gq, sizeof(double) * (size_t)g.n * ctx->DP * ctx->DP, hipMemcpyDeviceToDevice, st);
    });
    return;
  }
  launch(ctx, "assemble", [&](hipStream_t st) {
    if (ctx->flags & RMHMC_FLAG_FP32_METRIC) {  // precision experiment: fp32 matrix cores for the metric only
      if (ctx->big) {
        hipLaunchKernelGGL((k_assemble_f32<4>), dim3((unsigned)((g.n + 3) / 4), ctx->npairs), dim3(256), 0, st, ctx->dd, g.n, g.ch.phase, v,
                           g.ch.Gq, ctx->nbk);
      } else {
        NB_SWITCH(ctx, hipLaunchKernelGGL((k_assemble_f32<NB_>), dim3((unsigned)((g.n + 3) / 4)), dim3(256), 0, st, ctx->dd, g.n,
                                          g.ch.phase, v, g.ch.Gq, 1));
      }
      return;
    }
    if (ctx->big) {
      hipLaunchKernelGGL(k_assemble_pair<false>, dim3((unsigned)((g.n + 3) / 4), ctx->npairs - ctx->nbk), dim3(256), 0, st, ctx->dd, g.n,
                         g.ch.phase, v, g.ch.Gq);
      hipLaunchKernelGGL(k_assemble_pair<true>, dim3((unsigned)((g.n + 3) / 4), ctx->nbk), dim3(256), 0, st, ctx->dd, g.n, g.ch.phase, v,
                         g.ch.Gq);
      return;
    }
    if (ctx->fsplit > 1) {  // small batch: row ranges into planes, summed in a fixed order
      const size_t plane = (size_t)g.n * ctx->DP * ctx->DP;
      dim3 grid((unsigned)((g.n + 3) / 4), (unsigned)ctx->fsplit);
      NB_SWITCH(ctx, hipLaunchKernelGGL((k_assemble<NB_>), grid, dim3(256), 0, st, ctx->dd, g.n, g.ch.phase, v, g.Gpart, plane));
      hipLaunchKernelGGL(k_sum_planes, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, st, g.ch.Gq, g.Gpart, ctx->fsplit, plane, plane);
      return;
    }
    dim3 grid((unsigned)((g.n + 3) / 4));
    NB_SWITCH(ctx, hipLaunchKernelGGL((k_assemble<NB_>), grid, dim3(256), 0, st, ctx->dd, g.n, g.ch.phase, v, g.ch.Gq, (size_t)0));
  });
}

// q partials of u' dG/dw_d u for every chain (u = ch.uq, w as given); summed by k_mom_update / k_mom_final.
// cmode (generic path): 1 = first pass at this w, c is computed and kept; 2 = c of this w is at hand (k_mompass in kernels.hip.h)
void launch_mompass(rmhmc_ctx* ctx, Group& g, const double* w, int cmode) {
  launch(ctx, "mompass", [&](hipStream_t st) {
    if (!ctx->opt.ccache) cmode = 0;
    if (ctx->big) {
      dim3 grid((unsigned)((g.n + 15) / 16), ctx->nsplit);
      switch (cmode) {
        case 1: hipLaunchKernelGGL(k_mompass_big<1>, grid, dim3(256), 0, st, ctx->dd, g.n, ctx->nsplit, ctx->nbk, w, g.ch.uq, g.ch.qpart, g.ctile); break;
        case 2: hipLaunchKernelGGL(k_mompass_big<2>, grid, dim3(256), 0, st, ctx->dd, g.n, ctx->nsplit, ctx->nbk, w, g.ch.uq, g.ch.qpart, g.ctile); break;
        default: hipLaunchKernelGGL(k_mompass_big<0>, grid, dim3(256), 0, st, ctx->dd, g.n, ctx->nsplit, ctx->nbk, w, g.ch.uq, g.ch.qpart, g.ctile); break;
      }
      return;
    }
    dim3 grid((unsigned)((g.n + 63) / 64), ctx->nsplit);
    switch (cmode) {
      case 1:  // first pass of a step at this w: the tiles are at hand unless the chain has just rejected a proposal (k_mompass<.., 3>)
        if (ctx->opt.cdyn) { NB_SWITCH(ctx, hipLaunchKernelGGL((k_mompass<NB_, 3>), grid, dim3(256), 0, st, ctx->dd, g.n, ctx->nsplit, w, g.ch.uq, g.ch.qpart, g.ctile, g.ch.cstale)); }
        else { NB_SWITCH(ctx, hipLaunchKernelGGL((k_mompass<NB_, 1>), grid, dim3(256), 0, st, ctx->dd, g.n, ctx->nsplit, w, g.ch.uq, g.ch.qpart, g.ctile)); }
        break;
      case 2: NB_SWITCH(ctx, hipLaunchKernelGGL((k_mompass<NB_, 2>), grid, dim3(256), 0, st, ctx->dd, g.n, ctx->nsplit, w, g.ch.uq, g.ch.qpart, g.ctile)); break;
      default: NB_SWITCH(ctx, hipLaunchKernelGGL((k_mompass<NB_, 0>), grid, dim3(256), 0, st, ctx->dd, g.n, ctx->nsplit, w, g.ch.uq, g.ch.qpart, g.ctile)); break;
    }
  });
}

// The evaluation's momentum pass and the trace product are both X' R over the same rows and c tiles: on the generic int8 path with c tiles the
// leverage GEMM runs first and k_mompass_trv does both products in one pass (fused_trace); otherwise k_trvec follows the GEMM.
static bool fused_trace(const rmhmc_ctx* ctx, const Group& g) { return ctx->i8 && !ctx->big && g.ctile != nullptr && ctx->opt.ccache; }

// part: 0 everything; 1 the leverage GEMM alone (h -> rv0); 2 the reduction of the trace partials alone
void launch_leverage(rmhmc_ctx* ctx, Group& g, int part = 0) {
  if (ctx->i8 && part == 2) {
    launch(ctx, "small", [&](hipStream_t st) {
      hipLaunchKernelGGL(k_reduce_tr, dim3((unsigned)g.n), dim3(64), 0, st, ctx->D, ctx->DP, g.ch, g.ch.gpart, ctx->nsplit);
    });
    return;
  }
  if (ctx->i8) {  // h_n as the transposed sliced GEMM, then tr = X' (c .* h) on the fp64 matrix cores
    launch(ctx, "qsplit", [&](hipStream_t st) { I8_SWITCH(ctx, (launch_leverage_i8_t<S_, WN_, TN_>(ctx, g, st, 0))); });
    // The leverages h_n = x_n' G^-1 x_n enter the trace term only, which steers the momentum and appears in no Hamiltonian: like the metric
    // of an inner position iterate they are summed from the S - 1 most significant slices of the same operands (15 slice products
    // instead of 21; h to ~3e-12 norm-wise, theta / p after a step move by < 1e-11; RMHMC_FLAG_INT8_INNER_FULL: all S) - unless the
    // data set has so few rows per column that the metric is ill-conditioned (Plan::i8_lev_full)
    const int suse = (ctx->i8_inner_drop && ctx->i8S == 6 && !ctx->i8_lev_full) ? 5 : ctx->i8S;
    launch(ctx, "leverage_i8", [&](hipStream_t st) { I8_SWITCH_S(suse, (launch_leverage_i8_t<S_, WN_, TN_>(ctx, g, st, 1))); });
    if (part == 1) return;
    launch(ctx, "trvec", [&](hipStream_t st) {
      if (ctx->big) {  // rv0 holds h (one "pair" plane), the large-D trace kernel multiplies by c itself
        dim3 grid((unsigned)((g.n + 15) / 16), ctx->nsplit);
        hipLaunchKernelGGL(k_trace_big, grid, dim3(256), 0, st, ctx->dd, g.n, ctx->nsplit, ctx->nbk, 1, g.ch.rv2, g.ch.rv0, g.ch.gpart);
        return;
      }
      dim3 grid((unsigned)((g.n + 63) / 64), ctx->nsplit);
      NB_SWITCH(ctx, hipLaunchKernelGGL((k_trvec<NB_>), grid, dim3(256), 0, st, ctx->dd, g.n, ctx->nsplit, g.ch.rv0, g.ch.gpart, (const d4*)g.ctile));
    });
    launch(ctx, "small", [&](hipStream_t st) {
      hipLaunchKernelGGL(k_reduce_tr, dim3((unsigned)g.n), dim3(64), 0, st, ctx->D, ctx->DP, g.ch, g.ch.gpart, ctx->nsplit);
    });
    return;
  }
  if (ctx->big) {  // per block pair leverage contributions, then the trace GEMM over 16 chains per workgroup
    double* hpart = ctx->d_hpart;  // [pair][n][Mp]
    launch(ctx, "leverage", [&](hipStream_t st) {
      hipLaunchKernelGGL(k_leverage_pair<false>, dim3((unsigned)((g.n + 3) / 4), ctx->npairs - ctx->nbk), dim3(256), 0, st, ctx->dd, g.n,
                         ctx->nbk, g.ch.phase, g.ch.trj.Ginv, hpart);
      hipLaunchKernelGGL(k_leverage_pair<true>, dim3((unsigned)((g.n + 3) / 4), ctx->nbk), dim3(256), 0, st, ctx->dd, g.n, ctx->nbk,
                         g.ch.phase, g.ch.trj.Ginv, hpart);
    });
    launch(ctx, "leverage", [&](hipStream_t st) {
      dim3 grid((unsigned)((g.n + 15) / 16), ctx->nsplit);
      hipLaunchKernelGGL(k_trace_big, grid, dim3(256), 0, st, ctx->dd, g.n, ctx->nsplit, ctx->nbk, ctx->npairs, g.ch.rv2, hpart, g.ch.gpart);
    });
    launch(ctx, "small", [&](hipStream_t st) {
      hipLaunchKernelGGL(k_reduce_tr, dim3((unsigned)g.n), dim3(64), 0, st, ctx->D, ctx->DP, g.ch, g.ch.gpart, ctx->nsplit);
    });
    return;
  }
  const int fs = std::min(ctx->fsplit, ctx->nsplit);  // (the partials go to gpart, which holds nsplit planes)
  launch(ctx, "leverage", [&](hipStream_t st) {
    dim3 grid((unsigned)((g.n + 3) / 4), (unsigned)fs);
    NB_SWITCH(ctx, hipLaunchKernelGGL((k_leverage<NB_>), grid, dim3(256), 0, st, ctx->dd, g.n, g.ch.phase, g.ch.trj.Ginv, g.ch.rv2,
                                      g.ch.trj.tr, g.ch.gpart));
  });
  if (fs > 1)
    launch(ctx, "small", [&](hipStream_t st) {
      hipLaunchKernelGGL(k_reduce_tr, dim3((unsigned)g.n), dim3(64), 0, st, ctx->D, ctx->DP, g.ch, g.ch.gpart, fs);
    });
}

// one wavefront (64-thread block) per chain
#define SMALL(ctx, g, name, kern, ...)                                                                     \
  launch(ctx, name, [&](hipStream_t st_) { hipLaunchKernelGGL(kern, dim3((unsigned)(g).n), dim3(64), 0, st_, __VA_ARGS__); })

// one 256-thread workgroup per chain (blocked dense algebra of the large-D path)
#define BIG(ctx, g, name, kern, ...)                                                                       \
  launch(ctx, name, [&](hipStream_t st_) { hipLaunchKernelGGL(kern, dim3((unsigned)(g).n), dim3(256), 0, st_, __VA_ARGS__); })

// Evaluate the point record at trj.w for every chain in phase 1 (rmhmc.py:134-161): v, r, c, log-joint partials -> G and gradient
// on the matrix cores -> factor / inverse / u = G^-1 p -> quadratic term -> leverage pass (trace term) -> momentum update.
// step: the run whose leapfrog step this evaluation ends (the explicit momentum half step :163 follows; the last position iterate's
// slices and G are at hand), or nullptr: evaluate only, which needs no run parameters.  want_G (large-D): copy G to d_Gcopy.
// mode 0: everything; 1: metric, factor, inverse, gradient, log joint only (simplified mMALA); 2: mode 1 + the trace term (full mMALA)
void eval_point_phases(rmhmc_ctx* ctx, Group& g, const Run* step, int mode = 0, bool want_G = false) {
  const double eps = step ? step->eps : 0.0;  // (read by the kernels below only when they advance, see the two calls)
  const bool delta = step && use_delta(ctx, *step, g);
  launch_rowpass<RP_F>(ctx, g, g.ch.trj.w, g.ch.rv0, g.ch.rv2, delta);
  if (ctx->big) SMALL(ctx, g, "small", k_finish_big, ctx->dd, g.ch, ctx->nsplit);
  launch_assemble(ctx, g, g.ch.rv0, false, delta);
  if (ctx->big) {
    if (want_G)
      (void)hipMemcpyAsync(ctx->d_Gcopy, g.ch.Gq, sizeof(double) * (size_t)g.n * ctx->DP * ctx->DP, hipMemcpyDeviceToDevice, ctx->stream);
    BIG(ctx, g, "factor", k_chol_big<1>, ctx->dd, g.ch, ctx->nbk, ctx->d_Wd, eps);  // (MODE 1 does not read eps: only MODE 0 solves for wq)
    BIG(ctx, g, "factor", k_inverse_big, ctx->dd, g.ch, ctx->nbk, ctx->d_Wd);
    SMALL(ctx, g, "small", k_ginv_matvec, ctx->D, ctx->DP, g.ch, g.ch.p);
  } else {
    launch(ctx, "factor", [&](hipStream_t st) {
      NB_SWITCH(ctx, hipLaunchKernelGGL((k_factor_full<NB_>), dim3((unsigned)g.n), dim3(64), 0, st, ctx->dd, g.ch, ctx->nsplit));
    });
  }
  if (mode == 1) return;  // simplified mMALA needs neither the quadratic nor the trace term
  if (mode == 2) {        // full mMALA: the trace term enters the drift, the quadratic term does not exist
    launch_leverage(ctx, g);
    return;
  }
  if (fused_trace(ctx, g)) {  // leverage GEMM first, then ONE pass for the quadratic term and the trace term
    launch_leverage(ctx, g, 1);
    launch(ctx, "mompass", [&](hipStream_t st) {
      dim3 grid((unsigned)((g.n + 63) / 64), ctx->nsplit);
      NB_SWITCH(ctx, hipLaunchKernelGGL((k_mompass_trv<NB_>), grid, dim3(256), 0, st, ctx->dd, g.n, ctx->nsplit, g.ch.uq, g.ch.qpart, g.ctile, g.ch.rv0, g.ch.gpart));
    });  // (k_mom_final below sums the trace partials itself)
  } else {
    launch_mompass(ctx, g, g.ch.trj.w, 2);  // (the row pass above has just stored c for trj.w)
    launch_leverage(ctx, g);
  }
  // (without advance k_mom_final leaves p alone: the half step h = tau eps / 2 is formed and not used)
  SMALL(ctx, g, "small", k_mom_final, ctx->D, ctx->DP, g.ch, eps, step ? 1 : 0, ctx->nsplit, fused_trace(ctx, g) ? g.ch.gpart : (const double*)nullptr);
}

// one-launch step / evaluation / folded global step for small batches (medium_step.hip.h).  Data rows per thread stay in registers
// when at most 64 doubles are needed for them.
// step: the run that advances, or nullptr: eval_only (the kernel reads K, eps and h = tau eps / 2 in its `!eval_only` parts alone)
template <int NB>
void launch_step_medium_nb(rmhmc_ctx* ctx, Group& g, hipStream_t st, int guards, const Run* step, int fold, const IterParams& ip) {
  const double eps = step ? step->eps : 0.0;
  const int K = step ? step->K : 0, eval_only = step ? 0 : 1;
  const int rpt = (ctx->Mp + 255) / 256;
  const dim3 grid((unsigned)g.n), block(256);
  const size_t lds = ctx->medium_lds;
  switch (rpt * 16 * NB <= 64 ? rpt : 0) {
    case 1: hipLaunchKernelGGL((k_step_medium<NB, 1>), grid, block, lds, st, ctx->dd, g.ch, eps, K, guards, eval_only, fold, ip); break;
    case 2: hipLaunchKernelGGL((k_step_medium<NB, 2>), grid, block, lds, st, ctx->dd, g.ch, eps, K, guards, eval_only, fold, ip); break;
    case 3: hipLaunchKernelGGL((k_step_medium<NB, (NB == 1 ? 3 : 0)>), grid, block, lds, st, ctx->dd, g.ch, eps, K, guards, eval_only, fold, ip); break;
    case 4: hipLaunchKernelGGL((k_step_medium<NB, (NB == 1 ? 4 : 0)>), grid, block, lds, st, ctx->dd, g.ch, eps, K, guards, eval_only, fold, ip); break;
    default: hipLaunchKernelGGL((k_step_medium<NB, 0>), grid, block, lds, st, ctx->dd, g.ch, eps, K, guards, eval_only, fold, ip); break;
  }
}
void launch_step_medium(rmhmc_ctx* ctx, Group& g, hipStream_t st, int guards, const Run* step, int fold, const IterParams& ip) {
  if (ctx->NB == 1) launch_step_medium_nb<1>(ctx, g, st, guards, step, fold, ip);
  else launch_step_medium_nb<2>(ctx, g, st, guards, step, fold, ip);
}

// One generalised leapfrog step for every chain in phase 1 (rmhmc.py:96-163).
void step_phases(rmhmc_ctx* ctx, const Run& run, Group& g) {
  const int D = ctx->D, DP = ctx->DP, K = run.K;
  const double eps = run.eps;
  const int guards = (ctx->flags & RMHMC_FLAG_GUARDS) ? 1 : 0;
  if (ctx->medium) {  // the whole step in one launch, one workgroup per chain
    launch(ctx, "medium", [&](hipStream_t st) { launch_step_medium(ctx, g, st, guards, &run, 0, IterParams{}); });
    return;
  }
  // c tiles of the chains whose last proposal was rejected (their trj has fallen back to cur): recomputed for them alone, so that the
  // first momentum pass finds every chain's tiles at hand
  if (!ctx->big && ctx->opt.cdyn && g.ctile && g.ch.stale_list)
    launch(ctx, "mompass", [&](hipStream_t st) {
      // row pieces of this kernel's own, and a SMALL grid whose wavefronts walk the list (8 x 64 chains at a time): a wavefront alone on its
      // SIMD takes ~4.3 us per 32-row block (load - product - exp latencies with nothing to hide them), and workgroups that only read the
      // count and return are not free either.  Measured at config 3 (~300 listed chains = 19 wavefront groups per step, one box,
      // tools/crs_sweep.sh): grid 32 x 16 (round 2: room for 2048 chains, the rest left to k_mompass<.., 3>) 75.6 us, 8 x 16 43, 8 x 32 29.3,
      // 8 x 64 31.9, 4 x 64 28.6, 2 x 128 34.1.
      const int rsplit = std::max(1, std::min(32, ctx->Mp / 32 / 4));
      dim3 grid((unsigned)std::min((g.n + 63) / 64, 8), (unsigned)rsplit);
      NB_SWITCH(ctx, hipLaunchKernelGGL((k_crestore<NB_>), grid, dim3(256), 0, st, ctx->dd, g.n, g.ch.phase, g.ch.trj.w, g.ctile, g.ch.cstale,
                                        g.ch.stale_list, g.ch.stale_count));
      // (the count is reset by k_pos_first, later in the step)
    });
  // implicit momentum half step: K fixed-point iterations (rmhmc.py:102-110).  D <= 64: the update that ends an iteration and the G^-1 PM
  // product that starts the next are one launch (k_mom_update_matvec), the last update is done by k_pos_first
  const bool fuse = !ctx->big;
  for (int it = 0; it < K; ++it) {
    if (it == 0 || !fuse) SMALL(ctx, g, "small", k_ginv_matvec, D, DP, g.ch, it == 0 ? g.ch.p : g.ch.PM);
    launch_mompass(ctx, g, g.ch.trj.w, it == 0 ? 1 : 2);
    if (!fuse) SMALL(ctx, g, "small", k_mom_update, D, DP, g.ch, eps, it == K - 1 ? 1 : 0, ctx->nsplit);
    else if (it < K - 1) SMALL(ctx, g, "small", k_mom_update_matvec, D, DP, g.ch, eps, ctx->nsplit);
  }
  // implicit position step: K fixed-point iterations (rmhmc.py:113-123); the first one re-uses the
  // stored factor of G(w)
  if (ctx->big) {
    SMALL(ctx, g, "small", k_ginv_matvec, D, DP, g.ch, g.ch.p);
    SMALL(ctx, g, "small", k_pos_first_big, D, DP, g.ch, eps);
  } else {
    SMALL(ctx, g, "factor", k_pos_first, D, DP, g.ch, eps, ctx->nsplit);
  }
  for (int it = 1; it < K; ++it) {
    launch_rowpass<RP_V>(ctx, g, g.ch.wq, g.ch.rv0, nullptr, use_delta_inner(ctx, run, g, it));
    const bool base = (it == 1 && use_delta_inner(ctx, run, g, 2)) || (it == K - 1 && use_delta(ctx, run, g));
    launch_assemble(ctx, g, g.ch.rv0, it < K - 1, use_delta_inner(ctx, run, g, it), base);
    if (ctx->big)
      BIG(ctx, g, "factor", k_chol_big<0>, ctx->dd, g.ch, ctx->nbk, ctx->d_Wd, eps);
    else
      launch(ctx, "factor", [&](hipStream_t st) {  // (the last iterate: accepted as the new w, position guard, in the same launch)
        NB_SWITCH(ctx, hipLaunchKernelGGL((k_factor_solve<NB_>), dim3((unsigned)g.n), dim3(64), 0, st, D, DP, g.ch, eps, it == K - 1 ? guards : -1));
      });
  }
  if (ctx->big || K < 2) SMALL(ctx, g, "small", k_pos_final, D, DP, g.ch, guards);
  // explicit momentum half step at the new point (rmhmc.py:134-163)
  eval_point_phases(ctx, g, &run);
}

IterParams iter_params(rmhmc_ctx* ctx, const Run& run, const IterBase& b) {
  IterParams ip{};
  ip.flags = ctx->flags;
  ip.L = run.L;
  ip.seed = run.seed;
  ip.chain_offset = run.chain_offset;
  ip.iter_limit = b.limit;
  ip.burn_in = b.burn_in;
  ip.S = b.S;
  ip.samples = b.samples;
  ip.orig = run.orig;  // chain ids and sample blocks through the position -> chain map
  if (b.explicit_rng) {
    ip.z_in = ctx->d_z; ip.ulen_in = ctx->d_ulen; ip.gdir_in = ctx->d_gdir; ip.uacc_in = ctx->d_uacc;
  }
  ip.done_count = b.count_done ? ctx->d_done : nullptr;
  ip.lower_L = (!ctx->big && !ctx->medium && !ctx->fused && run.sampler == RMHMC) ? 1 : 0;  // (k_factor_full is the only writer of trj.L there)
  return ip;
}

void launch_iter_begin(rmhmc_ctx* ctx, const Run& run, Group& g, const IterBase& b) {
  SMALL(ctx, g, "small", k_iter_begin, ctx->D, ctx->DP, g.ch, iter_params(ctx, run, b));
}
void launch_iter_end(rmhmc_ctx* ctx, const Run& run, Group& g, const IterBase& b) {
  SMALL(ctx, g, "small", k_iter_end, ctx->D, ctx->DP, g.ch, iter_params(ctx, run, b));
}

// plain HMC (hmc.py:38-84): begin / half step + position / gradient pass / half step / end
// step: the run whose trajectories these are, or nullptr: eval_only (the kernel reads eps in its `!eval_only` half steps alone)
template <int NB>
void launch_hmc_traj_nb(rmhmc_ctx* ctx, Group& g, const Run* step, hipStream_t st) {
  const double eps = step ? step->eps : 0.0;
  const int eval_only = step ? 0 : 1;
  const int rpt = (ctx->Mp + 255) / 256;  // data rows per thread; up to 4 of them stay in registers for the whole trajectory
  const dim3 grid((unsigned)g.n), block(256);
  switch (rpt <= 4 ? rpt : 0) {
    case 1: hipLaunchKernelGGL((k_hmc_traj<NB, 1>), grid, block, 0, st, ctx->dd, g.ch, eps, eval_only); break;
    case 2: hipLaunchKernelGGL((k_hmc_traj<NB, 2>), grid, block, 0, st, ctx->dd, g.ch, eps, eval_only); break;
    case 3: hipLaunchKernelGGL((k_hmc_traj<NB, 3>), grid, block, 0, st, ctx->dd, g.ch, eps, eval_only); break;
    case 4: hipLaunchKernelGGL((k_hmc_traj<NB, 4>), grid, block, 0, st, ctx->dd, g.ch, eps, eval_only); break;
    default: hipLaunchKernelGGL((k_hmc_traj<NB, 0>), grid, block, 0, st, ctx->dd, g.ch, eps, eval_only); break;
  }
}
void launch_hmc_traj(rmhmc_ctx* ctx, Group& g, const Run* step) {
  launch(ctx, "medium", [&](hipStream_t st) {
    if (ctx->NB == 1) launch_hmc_traj_nb<1>(ctx, g, step, st);
    else launch_hmc_traj_nb<2>(ctx, g, step, st);
  });
}

void launch_hmc_global_step(rmhmc_ctx* ctx, const Run& run, Group& g, const IterBase& b) {
  const double eps = run.eps;
  const IterParams ip = iter_params(ctx, run, b);
  SMALL(ctx, g, "small", k_hmc_begin, ctx->D, ctx->DP, g.ch, ip);
  if (ctx->hmc_traj) {  // the whole trajectory of every chain in one launch
    launch_hmc_traj(ctx, g, &run);
  } else {
    SMALL(ctx, g, "small", k_hmc_pre, ctx->D, ctx->DP, g.ch, eps);
    launch_rowpass<RP_G>(ctx, g, g.ch.trj.w, nullptr);
    SMALL(ctx, g, "small", k_hmc_post, ctx->dd, g.ch, eps, ctx->nsplit);
  }
  SMALL(ctx, g, "small", k_hmc_end, ctx->D, ctx->DP, g.ch, ip);
}

// HMC with the context's mass matrix (phmc.hip.h): head / gradient pass / tail, the generic launches on every context
#define PHMC_SWITCH(ctx, ...)                                     \
  switch ((ctx)->DP / 16) {                                       \
    case 1: { constexpr int NDB_ = 1; __VA_ARGS__; } break;       \
    case 2: { constexpr int NDB_ = 2; __VA_ARGS__; } break;       \
    case 3: { constexpr int NDB_ = 3; __VA_ARGS__; } break;       \
    case 4: { constexpr int NDB_ = 4; __VA_ARGS__; } break;       \
    case 8: { constexpr int NDB_ = 8; __VA_ARGS__; } break;       \
    case 12: { constexpr int NDB_ = 12; __VA_ARGS__; } break;     \
    default: { constexpr int NDB_ = 16; __VA_ARGS__; } break;     \
  }
void launch_phmc_global_step(rmhmc_ctx* ctx, const Run& run, Group& g, const IterBase& b) {
  const double eps = run.eps;
  const IterParams ip = iter_params(ctx, run, b);
  const PhmcMass pm{ctx->d_massL, ctx->d_massInv};
  const dim3 grid((unsigned)((g.n + 15) / 16)), block(256);
  launch(ctx, "phmc", [&](hipStream_t st) {
    PHMC_SWITCH(ctx, hipLaunchKernelGGL((k_phmc_head<NDB_>), grid, block, phmc_lds_bytes<NDB_>(), st, ctx->D, g.ch, ip, pm, eps));
  });
  launch_rowpass<RP_G>(ctx, g, g.ch.trj.w, nullptr);
  launch(ctx, "phmc", [&](hipStream_t st) {
    PHMC_SWITCH(ctx, hipLaunchKernelGGL((k_phmc_tail<NDB_>), grid, block, phmc_lds_bytes<NDB_>(), st, ctx->dd, g.ch, ip, pm, eps, ctx->nsplit));
  });
}

// ... on the tempered target (ais.hip.h): the head and the gradient pass as they are, the tail under run.beta
void launch_tphmc_global_step(rmhmc_ctx* ctx, const Run& run, Group& g, const IterBase& b) {
  const double eps = run.eps, beta = run.beta;
  const IterParams ip = iter_params(ctx, run, b);
  const PhmcMass pm{ctx->d_massL, ctx->d_massInv};
  const dim3 grid((unsigned)((g.n + 15) / 16)), block(256);
  launch(ctx, "phmc", [&](hipStream_t st) {
    PHMC_SWITCH(ctx, hipLaunchKernelGGL((k_phmc_head<NDB_>), grid, block, phmc_lds_bytes<NDB_>(), st, ctx->D, g.ch, ip, pm, eps));
  });
  launch_rowpass<RP_G>(ctx, g, g.ch.trj.w, nullptr);
  launch(ctx, "ais", [&](hipStream_t st) {
    PHMC_SWITCH(ctx, hipLaunchKernelGGL((k_tphmc_tail<NDB_>), grid, block, phmc_lds_bytes<NDB_>(), st, ctx->dd, g.ch, ip, pm, eps, ctx->nsplit, beta,
                                        ctx->d_ais_ll));
  });
}

// One global step of the batch g: transition start, one leapfrog step and transition end of every chain
void launch_global_step(rmhmc_ctx* ctx, const Run& run, Group& g, const IterBase& b) {
  if (run.sampler == HMC) { launch_hmc_global_step(ctx, run, g, b); return; }
  if (run.sampler == PHMC) { launch_phmc_global_step(ctx, run, g, b); return; }
  if (run.sampler == TPHMC) { launch_tphmc_global_step(ctx, run, g, b); return; }
  if (ctx->medium) {  // ... in ONE launch
    const int guards = (ctx->flags & RMHMC_FLAG_GUARDS) ? 1 : 0;
    const IterParams ip = iter_params(ctx, run, b);
    launch(ctx, "medium", [&](hipStream_t st) { launch_step_medium(ctx, g, st, guards, &run, 1, ip); });
    return;
  }
  launch_iter_begin(ctx, run, g, b);
  step_phases(ctx, run, g);
  launch_iter_end(ctx, run, g, b);
}

// Small-problem path: one launch = `nsteps` global steps of every chain (fused_small.hip.h).
void launch_fused(rmhmc_ctx* ctx, const Run& run, const IterBase& b, long long nsteps) {
  Group& g = ctx->batch;
  while (nsteps > 0) {
    const int chunk = (int)std::min<long long>(nsteps, 4096);
    FusedParams fp{};
    fp.ip = iter_params(ctx, run, b);
    fp.eps = run.eps; fp.K = run.K; fp.nsteps = chunk; fp.DPs = ctx->DP; fp.init_eval = 0;
    launch(ctx, "fused", [&](hipStream_t st) {
      hipLaunchKernelGGL(k_fused_small, dim3((unsigned)((g.n + FS_WAVES - 1) / FS_WAVES)), dim3(64 * FS_WAVES), ctx->fused_lds, st,
                         ctx->dd, g.ch, fp);
    });
    nsteps -= chunk;
    if (nsteps > 0) flow_tick(ctx, ctx->opt.inflight);  // (one launch = up to 4096 steps: at most four launches queued ahead)
  }
}

// fill helpers on the context's stream
void fill_int(rmhmc_ctx* ctx, int* p, int v, size_t n) {
  hipLaunchKernelGGL(k_fill_int, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, p, v, n);
}
void fill_ll(rmhmc_ctx* ctx, long long* p, long long v, size_t n) {
  hipLaunchKernelGGL(k_fill_ll, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, p, v, n);
}

// the first `cols` doubles of each of `rows` rows, src [rows][src_cols] -> dst [rows][dst_cols]: how row padding is added or stripped
int copy_rows(rmhmc_ctx* ctx, double* dst, size_t dst_cols, const double* src, size_t src_cols, size_t cols, size_t rows, hipMemcpyKind kind) {
  HIPCK(hipMemcpy2DAsync(dst, dst_cols * sizeof(double), src, src_cols * sizeof(double), cols * sizeof(double), rows, kind, ctx->stream));
  return RMHMC_OK;
}
// host [n][D] -> device [n][DP] (padding stays zero) and back
int upload_vec(rmhmc_ctx* ctx, double* dst, const double* src) {
  return copy_rows(ctx, dst, ctx->DP, src, ctx->D, ctx->D, ctx->n, hipMemcpyHostToDevice);
}
int download_vec(rmhmc_ctx* ctx, double* dst, const double* src) {
  return copy_rows(ctx, dst, ctx->D, src, ctx->DP, ctx->D, ctx->n, hipMemcpyDeviceToHost);
}
template <typename T>
int download(rmhmc_ctx* ctx, T* dst, const T* src, size_t count) {
  HIPCK(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
  return RMHMC_OK;
}
template <typename T>
int upload(rmhmc_ctx* ctx, T* dst, const T* src, size_t count) {
  HIPCK(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
  return RMHMC_OK;
}

int sync(rmhmc_ctx* ctx) {
  HIPCK(hipStreamSynchronize(ctx->stream));
  HIPCK(hipGetLastError());
  return RMHMC_OK;
}
// ... after work that was queued with code rc, which may have failed half way: the stream is drained on every path, and the launcher's
// code goes before the synchronise's
int sync_after(rmhmc_ctx* ctx, int rc) {
  const int rs = sync(ctx);
  return rc != RMHMC_OK ? rc : rs;
}

#define RC(x) do { int rc_ = (x); if (rc_ != RMHMC_OK) return rc_; } while (0)
// ... of every row-per-thread instantiation of the one-launch step
template <int NB, int... RPT>
int raise_lds_medium(rmhmc_ctx* ctx) {
  for (const void* k : {(const void*)k_step_medium<NB, RPT>...}) RC(raise_lds(ctx, k, MAX_LDS));
  return RMHMC_OK;
}

#define NEED_DATA(ctx)                                                              \
  do {                                                                              \
    if (!(ctx)) return fail(nullptr, RMHMC_ERR_INVALID, "null context");            \
    if (!(ctx)->have_data) return fail(ctx, RMHMC_ERR_INVALID, "rmhmc_set_data has not been called"); \
    HIPCK(hipSetDevice((ctx)->device));                                             \
  } while (0)

// upload w into trj.w, zero (or upload) p, mark every chain active, evaluate the record (asynchronous: callers sync before they
// read the downloads).  one_launch: by the one-launch step kernel where the context has it; want_G: see eval_point_phases
int eval_at(rmhmc_ctx* ctx, const double* w, const double* p, bool one_launch = false, bool want_G = false) {
  Group& g = ctx->batch;
  Chains& ch = g.ch;
  RC(upload_vec(ctx, ch.trj.w, w));
  if (p) RC(upload_vec(ctx, ch.p, p));
  else HIPCK(hipMemsetAsync(ch.p, 0, sizeof(double) * ctx->n * ctx->DP, ctx->stream));
  fill_int(ctx, ch.phase, 1, ctx->n);
  fill_int(ctx, ch.status, 0, ctx->n);
  if (one_launch && ctx->medium) {  // same arithmetic as inside the one-launch steps (bit-exact checkpoint / resume)
    launch(ctx, "medium", [&](hipStream_t st) { launch_step_medium(ctx, g, st, 0, nullptr, 0, IterParams{}); });
    return RMHMC_OK;
  }
  eval_point_phases(ctx, g, nullptr, 0, want_G);
  return RMHMC_OK;
}

// Run-time options that live in device-visible state.  The list of the chains that have just rejected a proposal (k_iter_end appends,
// k_crestore consumes) exists on the generic multi-launch path with c tiles when cdyn and crestore are on.
void apply_runtime_options(rmhmc_ctx* ctx) {
  Group& g = ctx->batch;
  const bool ok = !ctx->big && !ctx->medium && !ctx->fused && g.ctile && ctx->opt.cdyn && ctx->opt.crestore;
  g.ch.stale_list = ok ? ctx->stale_list_alloc : nullptr;
}

}  // namespace

// =================================================================================================
// C-ABI
// =================================================================================================
extern "C" {

const char* rmhmc_version(void) { return "rmhmc-hip 0.1 (gfx950, fp64 MFMA)"; }
const char* rmhmc_last_error(const rmhmc_ctx* ctx) { return ctx ? ctx->err : g_err; }

int rmhmc_create(rmhmc_ctx** out, int32_t device_id, int64_t M, int32_t D, int64_t n_chains, int32_t dtype, uint32_t flags) {
  return rmhmc_create_opts(out, device_id, M, D, n_chains, dtype, flags, nullptr, 0);
}

int rmhmc_create_opts(rmhmc_ctx** out, int32_t device_id, int64_t M, int32_t D, int64_t n_chains, int32_t dtype, uint32_t flags,
                      const rmhmc_option* opts, int32_t n_opts) {
  rmhmc_ctx* ctx = nullptr;  // for the macros: errors go to the global message
  // 1. the options
  Options opt{};
  if (n_opts < 0 || (n_opts > 0 && !opts)) return fail(nullptr, RMHMC_ERR_INVALID, "rmhmc_create_opts: bad option array");
  for (int i = 0; i < n_opts; ++i) {
    const OptionDesc* d = find_option(opts[i].key);
    switch (check_option(d, opts[i].value, true)) {
      case OPT_UNKNOWN: return fail(nullptr, RMHMC_ERR_INVALID, std::string("rmhmc_create_opts: unknown option '") + (opts[i].key ? opts[i].key : "(null)") + "'");
      case OPT_RANGE: return fail(nullptr, RMHMC_ERR_INVALID, std::string("rmhmc_create_opts: value out of range for option '") + d->key + "'");
      default: opt.*(d->slot) = opts[i].value; break;
    }
  }
  // 2. the arguments, before any device call
  if (!out) return fail(nullptr, RMHMC_ERR_INVALID, "rmhmc_create: bad shape");
  if (const PlanCheck chk = plan_check(M, D, n_chains, dtype, flags); chk.code != RMHMC_OK) return fail(nullptr, chk.code, chk.msg);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, RMHMC_ERR_NO_DEVICE, "rmhmc_create: no HIP device available (this library has no CPU fallback)");
  if (device_id < 0 || device_id >= ndev) return fail(nullptr, RMHMC_ERR_NO_DEVICE, "rmhmc_create: device ordinal out of range");
  HIPCK(hipSetDevice(device_id));
  hipDeviceProp_t prop;
  HIPCK(hipGetDeviceProperties(&prop, device_id));
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
    return fail(nullptr, RMHMC_ERR_NO_DEVICE, std::string("rmhmc_create: kernels are built for gfx950 only, device is ") + prop.gcnArchName);
  // 3. every shape (plan.h)
  ctx = new rmhmc_ctx();
  static_cast<Plan&>(*ctx) = make_plan(M, D, n_chains, flags, opt);
  ctx->device = device_id;
  ctx->flags = flags; ctx->opt = opt;
  ctx->i8 = ctx->i8_requested;
  if (flags & RMHMC_FLAG_INT8_INNER_FULL) ctx->i8_inner_drop = 0;
  // 4. the allocations the plan asks for, and the LDS limits of the kernels it selects
  int rc = RMHMC_OK;
  auto body = [&]() -> int {
    HIPCK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    ctx->flow.resize(4);  // flow control events (flow_tick)
    for (auto& e : ctx->flow) { e = nullptr; HIPCK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); }
    const size_t n = n_chains, DP = ctx->DP, Mp = ctx->Mp;
    double *Xr, *Xt, *t;
    RC(dalloc(ctx, &Xr, Mp * DP)); RC(dalloc(ctx, &Xt, DP * Mp)); RC(dalloc(ctx, &t, Mp));
    ctx->dd.Xr = Xr; ctx->dd.Xt = Xt; ctx->dd.t = t;
    ctx->dd.M = (int)M; ctx->dd.Mp = ctx->Mp; ctx->dd.D = D; ctx->dd.DP = ctx->DP; ctx->dd.nblk = ctx->nblk;  // (kernel arguments)
    Group& g = ctx->batch;
    Chains& ch = g.ch;
    g.n = ch.n = (int)n;
    for (Rec* r : {&ch.cur, &ch.trj}) {
      RC(dalloc(ctx, &r->w, n * DP)); RC(dalloc(ctx, &r->grad, n * DP)); RC(dalloc(ctx, &r->tr, n * DP));
      RC(dalloc(ctx, &r->L, n * DP * DP)); RC(dalloc(ctx, &r->Ginv, n * DP * DP));
      RC(dalloc(ctx, &r->ljl, n)); RC(dalloc(ctx, &r->hld, n));
    }
    RC(dalloc(ctx, &ch.p, n * DP)); RC(dalloc(ctx, &ch.p0, n * DP)); RC(dalloc(ctx, &ch.Hcur, n)); RC(dalloc(ctx, &ch.Hprop, n));
    RC(dalloc(ctx, &ch.tau, n)); RC(dalloc(ctx, &ch.steps_left, n)); RC(dalloc(ctx, &ch.phase, n)); RC(dalloc(ctx, &ch.status, n)); RC(dalloc(ctx, &ch.cstale, n));
    RC(dalloc(ctx, &ch.stale_list, n)); RC(dalloc(ctx, &ch.stale_count, (size_t)1));
    ctx->stale_list_alloc = ch.stale_list;
    RC(dalloc(ctx, &ch.nsteps_last, n)); RC(dalloc(ctx, &ch.iter, n)); RC(dalloc(ctx, &ch.accepted, n)); RC(dalloc(ctx, &ch.steps_done, n));
    RC(dalloc(ctx, &ch.wq, n * DP)); RC(dalloc(ctx, &ch.uq, n * DP)); RC(dalloc(ctx, &ch.PM, n * DP)); RC(dalloc(ctx, &ch.u0, n * DP));
    RC(dalloc(ctx, &ch.q, n * DP)); RC(dalloc(ctx, &ch.last, n * DP)); RC(dalloc(ctx, &ch.Gq, n * DP * DP));
    RC(dalloc(ctx, &ch.rv0, n * Mp)); RC(dalloc(ctx, &ch.rv2, n * Mp));
    // partial planes of the row splits, c tiles
    RC(dalloc(ctx, &ch.qpart, (size_t)ctx->nsplit * n * DP));
    RC(dalloc(ctx, &ch.gpart, (size_t)ctx->nsplit * n * DP));
    RC(dalloc(ctx, &ch.ljl_part, n * ctx->nsplit));
    if (ctx->opt.ccache) RC(dalloc(ctx, &g.ctile, (size_t)((n + 15) / 16) * (Mp / 16) * 64));
    if (ctx->i8_requested) {
      g.nCp = ctx->nCp;
      const size_t S = ctx->i8S, NPp = ctx->NPp, nks = ctx->i8_nks, nkp = ctx->i8_nkp, NRp = ctx->i8_NRp, nCp = ctx->nCp;
      std::vector<short> pa(NPp, 0), pb(NPp, 0);
      for (int a = 0, q = 0; a < D; ++a)  // rows of the lower triangle
        for (int b = 0; b <= a; ++b, ++q) { pa[q] = (short)a; pb[q] = (short)b; }
      short *d_pa, *d_pb; double* d_scale;
      RC(dalloc(ctx, &d_pa, NPp)); RC(dalloc(ctx, &d_pb, NPp)); RC(dalloc(ctx, &d_scale, NPp));
      RC(dalloc(ctx, &ctx->d_ze, NPp));
      HIPCK(hipMemcpyAsync(d_pa, pa.data(), NPp * sizeof(short), hipMemcpyHostToDevice, ctx->stream));
      HIPCK(hipMemcpyAsync(d_pb, pb.data(), NPp * sizeof(short), hipMemcpyHostToDevice, ctx->stream));
      RC(sync(ctx));
      int* d_cexp;
      RC(dalloc(ctx, &d_cexp, DP));
      RC(dalloc(ctx, &ctx->d_cmin, DP)); RC(dalloc(ctx, &ctx->d_cmax, DP));
      ctx->pairs = I8Pairs{d_pa, d_pb, d_scale, ctx->NP, ctx->NPp, d_cexp};  // (kernel arguments)
      RC(dalloc(ctx, &ctx->d_Zs, S * nks * NPp * 32));
      RC(dalloc(ctx, &ctx->d_Zt, S * nkp * NRp * 32));
      RC(dalloc(ctx, &ctx->d_zre, NRp)); RC(dalloc(ctx, &ctx->d_zscale, NRp));
      // slice planes and accumulators of the batch
      RC(dalloc(ctx, &g.Vs, S * nks * nCp * 32));
      RC(dalloc(ctx, &g.vbad, nCp));
      RC(dalloc(ctx, &g.vexp, nCp));
      RC(dalloc(ctx, &g.vexp_d, nCp)); RC(dalloc(ctx, &g.rebase, nCp)); RC(dalloc(ctx, &g.dmax, (size_t)1));
      RC(dalloc(ctx, &g.dcount, (size_t)6));  // (before any graph is captured: every delta launch carries the pointer)
      if (!ctx->big) { ch.i8_vbad = g.vbad; ch.i8_dmax = g.dmax; }
      if (ctx->gbase) RC(dalloc(ctx, &g.Gbase, n * DP * DP));
      RC(dalloc(ctx, &g.Qs, S * nkp * nCp * 32));
      RC(dalloc(ctx, &g.qscale, nCp));
      if (ctx->tail_acc) RC(dalloc(ctx, &g.Tq, (size_t)ctx->tail_pieces * S * nCp * 32 * ctx->tail_blocks));
      if (ctx->ksplit_l > 1) RC(dalloc(ctx, &g.Rpart, (size_t)ctx->ksplit_l * n * Mp));
      // every instantiation the context can launch: its own slice count, at 6 slices also the 5 and 4 of the inner and delta assemblies
      for (int sv = ctx->i8S == 6 ? 4 : ctx->i8S; sv <= ctx->i8S; ++sv)
        I8_SWITCH_S(sv, {
          // (the instantiation's own, fixed size: these kernels also hold a few KB of static LDS, and static + dynamic must stay within 160 KB)
          constexpr int lds = i8_lds_bytes<S_, WN_, TN_>();
          RC(raise_lds(ctx, k_assemble_i8<S_, WN_, TN_>, lds));
          if constexpr (i8_zdirect_tile(S_, WN_, TN_)) if (i8_zdirect_on(ctx->opt.i8_zdirect, S_)) {
            RC(raise_lds(ctx, k_assemble_i8<S_, WN_, TN_, true>, (i8_lds_bytes<S_, WN_, TN_, true>())));
            RC(raise_lds(ctx, k_leverage_i8<S_, WN_, TN_, true>, (i8_lds_bytes<S_, WN_, TN_, true>())));
          }
          RC(raise_lds(ctx, k_leverage_i8<S_, WN_, TN_>, lds));
          RC(raise_lds(ctx, k_assemble_i8_tail<S_>, (i8_lds_bytes<S_, 1, 1>())));
        });
      if (ctx->i8S == 6) {  // the one-launch delta assembly (launch_assemble_i8_delta): dynamic LDS of its widest instantiation
        constexpr int lds_sel = std::max({i8_lds_bytes<6, 4, 1>(), i8_lds_bytes<4, 4, 1>(), i8_lds_bytes<4, 4, 1, true>(), i8_lds_bytes<5, 4, 1, true>()});
        RC(raise_lds(ctx, k_assemble_i8_sel<4, 1, 0>, lds_sel));
        RC(raise_lds(ctx, k_assemble_i8_sel<4, 1, 1>, lds_sel));
        RC(raise_lds(ctx, k_assemble_i8_sel<4, 1, 2>, lds_sel));
        RC(raise_lds(ctx, k_assemble_i8_sel<4, 1, 3>, lds_sel));
        RC(raise_lds(ctx, k_assemble_i8_tail_sel, std::max((i8_lds_bytes<6, 1, 1>()), (i8_lds_bytes<4, 1, 1>()))));
      }
    }
    if (ctx->gpart_planes) RC(dalloc(ctx, &g.Gpart, (size_t)ctx->gpart_planes * n * DP * DP));
    RC(dalloc(ctx, &ctx->d_z, n * (size_t)D)); RC(dalloc(ctx, &ctx->d_ulen, n)); RC(dalloc(ctx, &ctx->d_gdir, n)); RC(dalloc(ctx, &ctx->d_uacc, n));
    if (ctx->big) RC(dalloc(ctx, &ctx->d_Wd, n * (size_t)ctx->nbk * 4096));
    if (ctx->hpart_at_create) RC(dalloc(ctx, &ctx->d_hpart, (size_t)ctx->npairs * n * Mp));
    fill_int(ctx, ch.cstale, 1, n);  // (no c tiles yet; the first evaluation clears it)
    RC(dalloc(ctx, &ctx->d_nsteps, n)); RC(dalloc(ctx, &ctx->d_dir, n)); RC(dalloc(ctx, &ctx->d_done, 1)); RC(dalloc(ctx, &ctx->d_steps0, n));
    RC(dalloc(ctx, &ctx->d_miniter, 1));
    RC(dalloc(ctx, &ctx->d_orig, n)); RC(dalloc(ctx, &ctx->d_T, 2 * n));
    if (ctx->medium) RC(ctx->NB == 1 ? (raise_lds_medium<1, 0, 1, 2, 3, 4>(ctx)) : (raise_lds_medium<2, 0, 1, 2>(ctx)));
    if (ctx->fused) RC(raise_lds(ctx, k_fused_small, MAX_LDS));
    RC(sync(ctx));
    return RMHMC_OK;
  };
  rc = body();
  if (rc != RMHMC_OK) {
    snprintf(g_err, 512, "%s", ctx->err);
    rmhmc_destroy(ctx);
    return rc;
  }
  apply_runtime_options(ctx);
  *out = ctx;
  return RMHMC_OK;
}

void rmhmc_destroy(rmhmc_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  for (auto& e : ctx->flow) if (e) (void)hipEventDestroy(e);
  for (auto& kv : ctx->events) for (auto& e : kv.second) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  for (auto& e : ctx->pool) { (void)hipEventDestroy(e.a); (void)hipEventDestroy(e.b); }
  for (void* p : ctx->allocs) (void)hipFree(p);
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

int rmhmc_set_option(rmhmc_ctx* ctx, const char* key, int64_t value) {
  if (!ctx) return fail(nullptr, RMHMC_ERR_INVALID, "set_option: null context");
  const OptionDesc* d = find_option(key);
  switch (check_option(d, value, false)) {
    case OPT_UNKNOWN: return fail(ctx, RMHMC_ERR_INVALID, std::string("set_option: unknown option '") + (key ? key : "(null)") + "'");
    case OPT_CREATE_ONLY: return fail(ctx, RMHMC_ERR_INVALID, std::string("set_option: '") + key + "' shapes the context and can only be given to rmhmc_create_opts");
    case OPT_RANGE: return fail(ctx, RMHMC_ERR_INVALID, std::string("set_option: value out of range for '") + key + "'");
    case OPT_OK: break;
  }
  HIPCK(hipSetDevice(ctx->device));
  HIPCK(hipStreamSynchronize(ctx->stream));
  ctx->opt.*(d->slot) = value;
  apply_runtime_options(ctx);
  if (ctx->stale_list_alloc) {  // a list left over from a run with the other setting must not be consumed
    HIPCK(hipMemsetAsync(ctx->batch.ch.stale_count, 0, sizeof(int), ctx->stream));
    // (every chain's tiles count as stale: the next first pass recomputes them.  A second line of defence: k_iter_end sets the flag on
    //  every rejection and the RP_F row pass clears it whatever the options are, so the flags are exact without this fill too)
    fill_int(ctx, ctx->batch.ch.cstale, 1, ctx->n);
    HIPCK(hipStreamSynchronize(ctx->stream));
  }
  return RMHMC_OK;
}
int rmhmc_get_option(rmhmc_ctx* ctx, const char* key, int64_t* value_out) {
  if (!ctx || !value_out) return fail(ctx, RMHMC_ERR_INVALID, "get_option: null pointer");
  const OptionDesc* d = find_option(key);
  if (!d) return fail(ctx, RMHMC_ERR_INVALID, std::string("get_option: unknown option '") + (key ? key : "(null)") + "'");
  *value_out = ctx->opt.*(d->slot);
  return RMHMC_OK;
}
int rmhmc_options(rmhmc_ctx* ctx, char* buf, size_t len) {
  if (!ctx || !buf || !len) return fail(ctx, RMHMC_ERR_INVALID, "options: bad argument");
  std::string o;
  for (const OptionDesc& d : kOptions) o += (o.empty() ? "" : " ") + std::string(d.key) + "=" + std::to_string(ctx->opt.*(d.slot));
  snprintf(buf, len, "%s", o.c_str());
  return RMHMC_OK;
}

int rmhmc_device_info(rmhmc_ctx* ctx, char* buf, size_t len) {
  if (!ctx || !buf) return fail(ctx, RMHMC_ERR_INVALID, "device_info: bad argument");
  hipDeviceProp_t prop;
  HIPCK(hipGetDeviceProperties(&prop, ctx->device));
  snprintf(buf, len, "%s %s, %d CUs, %.0f MHz, %.1f GiB; M=%lld (padded %d) D=%d (padded %d, %d MFMA tiles) chains=%lld%s",
           prop.name, prop.gcnArchName, prop.multiProcessorCount, prop.clockRate / 1000.0, prop.totalGlobalMem / 1073741824.0,
           (long long)ctx->M, ctx->Mp, ctx->D, ctx->DP, ctx->NB * (ctx->NB + 1) / 2, (long long)ctx->n,
           ctx->fused ? ", fused small-problem path" : ctx->medium ? ", one-launch step" : ctx->big ? ", blocked large-D path" : "");
  if (ctx->i8_requested) {
    const size_t k = strlen(buf);
    snprintf(buf + k, len > k ? len - k : 0, "; int8 metric path %d slices: %s (certificate %.2e%s)", ctx->i8S,
             ctx->i8 ? "active" : "NOT certified for this data, fp64 matrix cores used", ctx->i8_bound,
             ctx->have_data ? "" : ", no data yet");
  }
  {
    const size_t k = strlen(buf);
    if (len > k + 12) {
      snprintf(buf + k, len - k, "; options: ");
      const size_t k2 = strlen(buf);
      (void)rmhmc_options(ctx, buf + k2, len - k2);
    }
  }
  return RMHMC_OK;
}

int rmhmc_set_data(rmhmc_ctx* ctx, const double* X, const double* t, double alpha) {
  if (!ctx || !X || !t || !(alpha > 0)) return fail(ctx, RMHMC_ERR_INVALID, "set_data: bad argument");
  HIPCK(hipSetDevice(ctx->device));
  const size_t M = ctx->M, D = ctx->D, DP = ctx->DP, Mp = ctx->Mp;
  std::vector<double> xr(Mp * DP, 0.0), xt(DP * Mp, 0.0), tt(Mp, 0.0);
  for (size_t n = 0; n < M; ++n) {
    for (size_t d = 0; d < D; ++d) {
      xr[n * DP + d] = X[n * D + d];
      xt[d * Mp + n] = X[n * D + d];
    }
    tt[n] = t[n];
  }
  HIPCK(hipMemcpyAsync((void*)ctx->dd.Xr, xr.data(), xr.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCK(hipMemcpyAsync((void*)ctx->dd.Xt, xt.data(), xt.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  HIPCK(hipMemcpyAsync((void*)ctx->dd.t, tt.data(), tt.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  if (ctx->i8_requested) {  // fixed operand of the int8 metric path: slices of x_a x_b for every column pair
    std::vector<int> cexp(DP, 0);  // power-of-two column equilibration of the leverage pass: max_n |x_na| < 2^cexp[a]
    std::vector<double> cmin(DP, 0.0), cmax(DP, 0.0);
    for (size_t d = 0; d < D; ++d) {
      double m = 0.0, lo = INFINITY;
      for (size_t n = 0; n < M; ++n) { const double a = std::fabs(X[n * D + d]); m = std::max(m, a); lo = std::min(lo, a); }
      if (m > 0.0 && m < 1e300) (void)std::frexp(m, &cexp[d]);
      if (m < 1e300) { cmin[d] = lo; cmax[d] = m; }
    }
    HIPCK(hipMemcpyAsync((void*)ctx->pairs.cexp, cexp.data(), sizeof(int) * DP, hipMemcpyHostToDevice, ctx->stream));
    HIPCK(hipMemcpyAsync(ctx->d_cmin, cmin.data(), sizeof(double) * DP, hipMemcpyHostToDevice, ctx->stream));
    HIPCK(hipMemcpyAsync(ctx->d_cmax, cmax.data(), sizeof(double) * DP, hipMemcpyHostToDevice, ctx->stream));
    RC(sync(ctx));  // (cexp is a local)
    hipLaunchKernelGGL(k_zmax, dim3((unsigned)ctx->pairs.NPp), dim3(256), 0, ctx->stream, ctx->dd.Xt, (int)M, (int)Mp, ctx->pairs, ctx->d_ze,
                       (double*)ctx->pairs.scale);
    const dim3 grid((unsigned)((ctx->i8_nks * 8 + 255) / 256), (unsigned)ctx->pairs.NPp);
    I8_SWITCH(ctx, hipLaunchKernelGGL((k_zsplit<S_>), grid, dim3(256), 0, ctx->stream, ctx->dd.Xt, (int)M, (int)Mp, ctx->pairs, ctx->d_ze,
                                      ctx->i8_nks, ctx->d_Zs); (void)WN_; (void)TN_);
    hipLaunchKernelGGL(k_zrowmax, dim3((unsigned)((ctx->i8_NRp + 255) / 256)), dim3(256), 0, ctx->stream, ctx->dd.Xr, (int)M, (int)D, (int)DP,
                       ctx->i8_NRp, ctx->pairs.cexp, ctx->d_zre, ctx->d_zscale);
    const dim3 gridt((unsigned)(ctx->i8_NRp / 32), (unsigned)ctx->i8_nkp);
    I8_SWITCH(ctx, hipLaunchKernelGGL((k_ztsplit<S_>), gridt, dim3(256), 0, ctx->stream, ctx->dd.Xr, (int)M, (int)DP, ctx->pairs, ctx->d_zre,
                                      ctx->i8_nkp, ctx->i8_NRp, ctx->d_Zt); (void)WN_; (void)TN_);
    HIPCK(hipGetLastError());
  }
  RC(sync(ctx));
  if (ctx->i8_requested) {
    // Certificate of the fixed-point assembly for THIS data (metric_i8.hip.h, "Error bound"): worst-case error of G_ab relative to
    // sqrt(G0_aa G0_bb), G0 = X'X/4 + I/alpha (the metric at w = 0), maximised over the column pairs.
    std::vector<int> ze(ctx->pairs.NP);
    HIPCK(hipMemcpy(ze.data(), ctx->d_ze, sizeof(int) * ze.size(), hipMemcpyDeviceToHost));
    std::vector<double> g0(D, 1.0 / alpha);
    for (size_t n = 0; n < M; ++n)
      for (size_t d = 0; d < D; ++d) g0[d] += 0.25 * X[n * D + d] * X[n * D + d];
    double bound = 0.0;
    for (size_t a = 0, q = 0; a < D; ++a)
      for (size_t b = 0; b <= a; ++b, ++q)
        bound = std::max(bound, std::ldexp((double)ctx->i8S * (double)M, ze[q] - 8 * ctx->i8S) / std::sqrt(g0[a] * g0[b]));
    // (delta assembly at the end of a step: the slice products dropped from the difference add to those dropped from the base matrix)
    if (ctx->opt.i8_delta && ctx->i8S == 6) bound *= (2.0 * ctx->i8S - 1.0) / ctx->i8S;
    ctx->i8_bound = bound;
    const bool ok = !(ctx->flags & RMHMC_FLAG_INT8_CERTIFY) || bound <= RMHMC_INT8_CERTIFY_TOL;
    if (!ok && ctx->big && !ctx->d_hpart) RC(dalloc(ctx, &ctx->d_hpart, (size_t)ctx->npairs * ctx->n * Mp));
    ctx->i8 = ok;  // not certified: this data set runs on the fp64 matrix cores (same context, same results to fp64 rounding)
    RC(sync(ctx));
  }
  ctx->alpha = alpha;
  ctx->dd.inv_alpha = 1.0 / alpha;
  ctx->dd.log_prior_const = -0.5 * std::log(2.0 * M_PI * alpha);
  ctx->have_data = true;
  ctx->chains_ready = false;
  return RMHMC_OK;
}

// ---- unit entry points --------------------------------------------------------------------------
int rmhmc_log_posterior(rmhmc_ctx* ctx, const double* w, double* ljl_out) {
  NEED_DATA(ctx);
  if (!w || !ljl_out) return fail(ctx, RMHMC_ERR_INVALID, "log_posterior: null pointer");
  ctx->chains_ready = false;
  RC(eval_at(ctx, w, nullptr));
  RC(download(ctx, ljl_out, ctx->batch.ch.trj.ljl, ctx->n));
  return sync(ctx);
}

int rmhmc_metric(rmhmc_ctx* ctx, const double* w, double* G_out, double* half_logdet_out, double* grad_out) {
  NEED_DATA(ctx);
  if (!w) return fail(ctx, RMHMC_ERR_INVALID, "metric: null pointer");
  ctx->chains_ready = false;
  const bool want_G = ctx->big && G_out;
  if (want_G && !ctx->d_Gcopy) RC(dalloc(ctx, &ctx->d_Gcopy, (size_t)ctx->n * ctx->DP * ctx->DP));
  RC(eval_at(ctx, w, nullptr, false, want_G));
  if (G_out)
    for (int64_t c = 0; c < ctx->n; ++c)  // strip the padding: [DP][DP] -> [D][D]
      HIPCK(hipMemcpy2DAsync(G_out + c * ctx->D * ctx->D, ctx->D * 8, (ctx->big ? ctx->d_Gcopy : ctx->batch.ch.Gq) + c * ctx->DP * ctx->DP, ctx->DP * 8, ctx->D * 8, ctx->D,
                             hipMemcpyDeviceToHost, ctx->stream));
  if (half_logdet_out) RC(download(ctx, half_logdet_out, ctx->batch.ch.trj.hld, ctx->n));
  if (grad_out) RC(download_vec(ctx, grad_out, ctx->batch.ch.trj.grad));
  RC(sync(ctx));
  if (G_out && ctx->i8) {  // the int8 assembly writes the lower triangle only
    const int64_t D = ctx->D;
    for (int64_t c = 0; c < ctx->n; ++c)
      for (int64_t a = 0; a < D; ++a)
        for (int64_t b = a + 1; b < D; ++b) G_out[(c * D + a) * D + b] = G_out[(c * D + b) * D + a];
  }
  return RMHMC_OK;
}

int rmhmc_metric_terms(rmhmc_ctx* ctx, const double* w, const double* p, double* trace_out, double* quad_out) {
  NEED_DATA(ctx);
  if (!w) return fail(ctx, RMHMC_ERR_INVALID, "metric_terms: null pointer");
  ctx->chains_ready = false;
  RC(eval_at(ctx, w, p));
  if (trace_out) RC(download_vec(ctx, trace_out, ctx->batch.ch.trj.tr));
  if (quad_out && p) RC(download_vec(ctx, quad_out, ctx->batch.ch.last));
  return sync(ctx);
}

int rmhmc_leapfrog(rmhmc_ctx* ctx, double* w, double* p, double eps, const int32_t* dir, const int32_t* nsteps, int32_t K,
                   double* half_logdet_out, int32_t* status_out) {
  NEED_DATA(ctx);
  if (!w || !p || !dir || !nsteps || K < 1) return fail(ctx, RMHMC_ERR_INVALID, "leapfrog: null pointer or K < 1");
  ctx->chains_ready = false;
  int maxs = 0;
  for (int64_t c = 0; c < ctx->n; ++c) {
    if (nsteps[c] < 0 || (dir[c] != 1 && dir[c] != -1)) return fail(ctx, RMHMC_ERR_INVALID, "leapfrog: nsteps >= 0 and dir = +-1 required");
    if (nsteps[c] > maxs) maxs = nsteps[c];
  }
  const Run run{RMHMC, 0, K, eps, 0, 0, nullptr};  // (no transitions: nothing draws a trajectory length from L)
  RC(upload(ctx, ctx->d_nsteps, nsteps, ctx->n));
  RC(upload(ctx, ctx->d_dir, dir, ctx->n));
  RC(eval_at(ctx, w, p));
  Group& g = ctx->batch;
  launch(ctx, "small", [&](hipStream_t st) {
    hipLaunchKernelGGL(k_set_leapfrog, dim3((unsigned)((g.n + 255) / 256)), dim3(256), 0, st, g.n, ctx->d_nsteps, ctx->d_dir, g.ch);
  });
  for (int s = 0; s < maxs; ++s) {
    step_phases(ctx, run, g);
    launch(ctx, "small", [&](hipStream_t st) {
      hipLaunchKernelGGL(k_park_finished, dim3((unsigned)((g.n + 255) / 256)), dim3(256), 0, st, g.n, g.ch);
    });
  }
  RC(download_vec(ctx, w, ctx->batch.ch.trj.w));
  RC(download_vec(ctx, p, ctx->batch.ch.p));
  if (half_logdet_out) RC(download(ctx, half_logdet_out, ctx->batch.ch.trj.hld, ctx->n));
  if (status_out) RC(download(ctx, status_out, ctx->batch.ch.status, ctx->n));
  return sync(ctx);
}

// every chain between transitions with its counters at zero, nobody done; synchronises
static int reset_chains(rmhmc_ctx* ctx) {
  Chains& ch = ctx->batch.ch;
  fill_int(ctx, ch.phase, 0, ctx->n);
  fill_int(ctx, ch.steps_left, 0, ctx->n);
  fill_int(ctx, ch.status, 0, ctx->n);
  fill_ll(ctx, ch.iter, 0, ctx->n);
  fill_ll(ctx, ch.accepted, 0, ctx->n);
  fill_ll(ctx, ch.steps_done, 0, ctx->n);
  HIPCK(hipMemsetAsync(ctx->d_done, 0, sizeof(int), ctx->stream));
  return sync(ctx);
}

// shared by transition / sample / chains_init: evaluate the record at theta0 and commit it as the
// current point of every chain.  By default the evaluation is that of the context's stepping path (same arithmetic as inside its
// steps); the samplers that step with the generic kernels whatever the context say which one-launch evaluations they may not get.
static int init_chains(rmhmc_ctx* ctx, const double* theta0_host /* [n][D] or NULL */, bool allow_fused = true, bool allow_medium = true) {
  Group& g = ctx->batch;
  std::vector<double> th;
  if (!theta0_host) {
    th.assign((size_t)ctx->n * ctx->D, 1e-3);  // rmhmc.py:27
    theta0_host = th.data();
  }
  if (ctx->fused && allow_fused) {  // the fused path evaluates its own initial record (same arithmetic as inside its steps)
    RC(upload_vec(ctx, g.ch.cur.w, theta0_host));
    FusedParams fp{};  // (init_eval returns before the kernel reads ip, eps or K: an evaluation needs no run parameters)
    fp.nsteps = 0; fp.DPs = ctx->DP; fp.init_eval = 1;
    launch(ctx, "fused", [&](hipStream_t st) {
      hipLaunchKernelGGL(k_fused_small, dim3((unsigned)((g.n + FS_WAVES - 1) / FS_WAVES)), dim3(64 * FS_WAVES), ctx->fused_lds, st,
                         ctx->dd, g.ch, fp);
    });
  } else {
    RC(eval_at(ctx, theta0_host, nullptr, allow_medium));
    SMALL(ctx, g, "small", k_commit_all, ctx->D, ctx->DP, g.ch);
  }
  return reset_chains(ctx);  // (synchronises: the theta0 staging vector goes out of scope)
}

// The read-back of a single transition, shared by rmhmc_transition, hmc_transition_body and rmhmc_mmala_transition: the current point
// into w, the optional outputs (NULL: not wanted, or the sampler has none), then the synchronise, which also drains the downloads the
// caller queued before it, and the accepted counter narrowed to int32.
static int transition_out(rmhmc_ctx* ctx, double* w, int32_t* accepted_out, int32_t* nsteps_out, double* H_cur_out, double* H_prop_out,
                          double* w_prop_out, double* p_prop_out, int32_t* status_out) {
  const Chains& ch = ctx->batch.ch;
  std::vector<long long> acc(ctx->n);
  RC(download_vec(ctx, w, ch.cur.w));
  RC(download(ctx, acc.data(), ch.accepted, ctx->n));
  if (nsteps_out) RC(download(ctx, nsteps_out, ch.nsteps_last, ctx->n));
  if (H_cur_out) RC(download(ctx, H_cur_out, ch.Hcur, ctx->n));
  if (H_prop_out) RC(download(ctx, H_prop_out, ch.Hprop, ctx->n));
  if (w_prop_out) RC(download_vec(ctx, w_prop_out, ch.trj.w));
  if (p_prop_out) RC(download_vec(ctx, p_prop_out, ch.p));
  if (status_out) RC(download(ctx, status_out, ch.status, ctx->n));
  RC(sync(ctx));
  if (accepted_out) for (int64_t c = 0; c < ctx->n; ++c) accepted_out[c] = (int32_t)acc[c];
  return RMHMC_OK;
}

int rmhmc_transition(rmhmc_ctx* ctx, double* w, const double* z, const double* u_len, const double* g_dir, const double* u_acc,
                     int32_t L, double eps, int32_t K, int32_t* accepted_out, int32_t* nsteps_out, double* H_cur_out,
                     double* H_prop_out, double* w_prop_out, double* p_prop_out, double* half_logdet_prop_out, int32_t* status_out) {
  NEED_DATA(ctx);
  if (!w || !z || !u_len || !g_dir || !u_acc || L < 1 || K < 1) return fail(ctx, RMHMC_ERR_INVALID, "transition: null pointer, L < 1 or K < 1");
  ctx->chains_ready = false;
  const Run run{RMHMC, L, K, eps, 0, 0, nullptr};  // (the randomness is the caller's: no seed)
  RC(init_chains(ctx, w));
  RC(upload(ctx, ctx->d_z, z, (size_t)ctx->n * ctx->D));
  RC(upload(ctx, ctx->d_ulen, u_len, ctx->n));
  RC(upload(ctx, ctx->d_gdir, g_dir, ctx->n));
  RC(upload(ctx, ctx->d_uacc, u_acc, ctx->n));
  const IterBase ib{1, 0, 0, nullptr, true, false};
  if (ctx->fused) {
    launch_fused(ctx, run, ib, L);
  } else {
    Group& g = ctx->batch;
    launch_iter_begin(ctx, run, g, ib);
    launch_iter_end(ctx, run, g, ib);  // trajectories of zero steps
    for (int s = 0; s < L; ++s) {
      step_phases(ctx, run, g);
      launch_iter_end(ctx, run, g, ib);
    }
  }
  if (half_logdet_prop_out) RC(download(ctx, half_logdet_prop_out, ctx->batch.ch.trj.hld, ctx->n));
  return transition_out(ctx, w, accepted_out, nsteps_out, H_cur_out, H_prop_out, w_prop_out, p_prop_out, status_out);
}

// ---- bulk entry points --------------------------------------------------------------------------
// The ~40 launches of one global step captured once into a hipGraph and replayed: the generic path is launch bound
// for small batches (config 1: 0.5 ms per step of one chain, nearly all of it launch latency).  Option graph = 0 disables.
struct StepGraph {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  ~StepGraph() {
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
  }
};
static bool step_graph_usable(const rmhmc_ctx* ctx, const Run& run, long long nsteps) {
  if (ctx->timing || nsteps < 8) return false;
  if (ctx->fused && run.sampler == RMHMC) return false;
  if (ctx->medium && run.sampler == RMHMC) return false;  // (the global step is ONE launch there: a one-node graph only costs its instantiation)
  return ctx->opt.graph != 0;
}
static bool build_step_graph(rmhmc_ctx* ctx, const Run& run, const IterBase& ib, StepGraph& sg) {
  if (hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) return false;
  launch_global_step(ctx, run, ctx->batch, ib);
  if (hipStreamEndCapture(ctx->stream, &sg.graph) != hipSuccess || !sg.graph) { (void)hipGetLastError(); return false; }
  if (hipGraphInstantiate(&sg.exec, sg.graph, nullptr, nullptr, 0) != hipSuccess) { (void)hipGetLastError(); sg.exec = nullptr; return false; }
  return true;
}
// nsteps global steps of the generic path (graph replay when it pays, plain launches otherwise)
static void run_generic_steps(rmhmc_ctx* ctx, const Run& run, const IterBase& ib, long long nsteps, StepGraph* sg) {
  if (sg && sg->exec) {
    for (long long s = 0; s < nsteps; ++s) { (void)hipGraphLaunch(sg->exec, ctx->stream); flow_tick(ctx); }
  } else {
    for (long long s = 0; s < nsteps; ++s) { launch_global_step(ctx, run, ctx->batch, ib); flow_tick(ctx); }
  }
}

// number of chains that reached the iteration limit and the completed transitions of the slowest chain, in one round trip
static int poll_progress(rmhmc_ctx* ctx, int* done, long long* min_iter) {
  HIPCK(hipMemsetAsync(ctx->d_miniter, 0xff, sizeof(unsigned long long), ctx->stream));
  hipLaunchKernelGGL(k_min_iter, dim3((unsigned)((ctx->n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->batch.ch.iter, (size_t)ctx->n, ctx->d_miniter);
  unsigned long long mi = 0;
  HIPCK(hipMemcpyAsync(done, ctx->d_done, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  HIPCK(hipMemcpyAsync(&mi, ctx->d_miniter, sizeof(mi), hipMemcpyDeviceToHost, ctx->stream));
  RC(sync(ctx));
  *min_iter = (long long)mi;
  return RMHMC_OK;
}

// rmhmc_set_progress: hand the caller the counters at a moment when every chain has completed at least `iters` transitions
static int report_progress(rmhmc_ctx* ctx, int event, long long iters) {
  std::vector<long long> acc(ctx->n), it(ctx->n);
  RC(download(ctx, acc.data(), ctx->batch.ch.accepted, ctx->n));
  RC(download(ctx, it.data(), ctx->batch.ch.iter, ctx->n));
  RC(sync(ctx));
  long long tot = 0, tit = 0;
  for (long long a : acc) tot += a;
  for (long long a : it) tit += a;
  ctx->progress_fn(event, iters, tot, tit, ctx->progress_user);
  return RMHMC_OK;
}
// Batches of several chains report without stopping anybody: whenever the host looks at the device anyway, the milestones the
// SLOWEST chain has passed since the last report are reported (once, with the largest of them).  Cutting a batch at every
// milestone, as the one-chain mode does to reproduce the reference's print-out exactly, would make every chain wait for the
// slowest fifty iterations at a time (+27 % at 8192 chains).
static bool progress_ticking(const rmhmc_ctx* ctx) { return ctx->progress_fn && ctx->progress_every > 0 && ctx->n > 1; }
// next: the sampling call's next milestone to report, or nullptr: a phase without reports (run_phase: none for ONE chain either)
static int progress_fire(rmhmc_ctx* ctx, long long* next, long long min_iter) {
  if (!next || !progress_ticking(ctx)) return RMHMC_OK;
  long long last = -1;
  while (*next <= min_iter) { last = *next; *next += ctx->progress_every; }
  if (last >= 0) RC(report_progress(ctx, RMHMC_EV_PROGRESS, last));
  return RMHMC_OK;
}

static int run_until_done(rmhmc_ctx* ctx, const Run& run, const IterBase& ib, long long min_steps, long long* progress_next) {
  // Every chain needs at least min_steps more global steps.  Afterwards the host looks at the device state and issues, each time,
  // as many steps as the slowest chain is certain to need: (limit - its completed transitions), a transition taking >= 1 step.
  // The remaining work shrinks geometrically (a transition averages (L+1)/2 steps), so a run costs O(log) host round trips
  // instead of one per 4 steps (thousands of syncs inside the TimeTaken window of the one-launch paths).
  int done = 0;
  long long s = min_steps, min_iter = 0;
  const long long poll = 4;
  const bool fused = ctx->fused && run.sampler == RMHMC;
  const bool ticking = progress_next && progress_ticking(ctx);
  const long long chunk = ticking ? std::max<long long>(8, ctx->progress_every * (run.L + 1) / 2) : min_steps;  // ~ one report per chunk
  StepGraph sg;
  if (!fused && step_graph_usable(ctx, run, std::min(min_steps, chunk))) (void)build_step_graph(ctx, run, ib, sg);
  for (long long left = min_steps; left > 0;) {
    const long long k = std::min(left, chunk);
    if (fused) launch_fused(ctx, run, ib, k);
    else run_generic_steps(ctx, run, ib, k, &sg);
    left -= k;
    if (ticking && left > 0) {
      RC(poll_progress(ctx, &done, &min_iter));
      RC(progress_fire(ctx, progress_next, min_iter));
    }
  }
  for (;;) {
    RC(poll_progress(ctx, &done, &min_iter));
    RC(progress_fire(ctx, progress_next, min_iter));
    if (done >= ctx->n) break;
    long long next = std::max(poll, ib.limit - min_iter);
    if (ticking) next = std::min(next, chunk);
    if (fused) launch_fused(ctx, run, ib, next);
    else run_generic_steps(ctx, run, ib, next, &sg);
    s += next;
    if (s > min_steps * (long long)run.L + 1000000) return fail(ctx, RMHMC_ERR_RUNTIME, "sampler did not terminate");
  }
  return RMHMC_OK;
}

// Every chain from exactly `from` to exactly ib.limit completed transitions.  With a progress callback and ONE chain the run is cut
// at the milestones first, first+every, ...: the callback gets the exact counters there, as the reference prints them, and the run goes
// on; the results do not depend on it (the randomness is keyed by chain and iteration).  Several chains: see progress_fire.
// A milestone that coincides with a phase boundary (burn_in + 1 completed transitions) is reported on the side of the burn-in banner
// where the reference prints it: rmhmc.py:38-45 prints at the TOP of the next iteration, i.e. after the banner of :194-196
// (at_from of phase B); hmc.py:85-94 prints at the bottom of the iteration itself, just before the banner (at_limit of phase A).
static int run_phase(rmhmc_ctx* ctx, const Run& run, const IterBase& ib, long long from, long long* progress_next, bool at_from = false, bool at_limit = false) {
  if (progress_next && ctx->progress_fn && ctx->progress_every > 0 && ctx->n == 1) {
    long long m = ctx->progress_first;
    if (from > m) m += ((from - m + ctx->progress_every - 1) / ctx->progress_every) * ctx->progress_every;   // first milestone >= from
    if (m == from) {
      if (at_from) RC(report_progress(ctx, RMHMC_EV_PROGRESS, m));
      m += ctx->progress_every;
    }
    for (; m < ib.limit || (at_limit && m == ib.limit); m += ctx->progress_every) {
      IterBase seg = ib;
      seg.limit = m;
      HIPCK(hipMemsetAsync(ctx->d_done, 0, sizeof(int), ctx->stream));
      RC(run_until_done(ctx, run, seg, m - from, progress_next));
      RC(report_progress(ctx, RMHMC_EV_PROGRESS, m));
      from = m;
    }
    HIPCK(hipMemsetAsync(ctx->d_done, 0, sizeof(int), ctx->stream));
  }
  if (ib.limit > from) RC(run_until_done(ctx, run, ib, ib.limit - from, progress_next));
  return RMHMC_OK;
}

// One global step on the first na chains only (na a multiple of 128 or n), on a narrowed copy of the batch: every kernel takes its
// chain count and its partial-plane strides from the batch it is handed, so producers and consumers agree.
static void launch_global_step_prefix(rmhmc_ctx* ctx, const Run& run, const IterBase& ib, int na) {
  Group g = ctx->batch;
  g.n = na; g.ch.n = na;
  if (g.nCp) g.nCp = (na + I8_BM - 1) / I8_BM * I8_BM;
  // (only the chain count and its int8 padding narrow.  Row ranges, k-split planes and row splits are the plan's, chosen for the
  // whole batch: every chain's sums keep their order, so the results are bit-identical to the unsorted run)
  launch_global_step(ctx, run, g, ib);
}

// Work-sorted phase B.  The trajectory lengths do not depend on the state (RandomStep = ceil(rand() L), rmhmc.py:89), so the number of
// leapfrog steps T_c every chain needs for its post-burn-in transitions is known beforehand.  With the chains laid out in order of
// decreasing T_c, the chains still running after s global steps are a prefix of the batch, and the launches of the tail shrink with it:
// the phase costs sum_c T_c chain-steps instead of n max_c T_c (8192 chains, 199 transitions: 791 global steps for a mean of 696, i.e.
// 12 % of the TimeTaken window spent on finished chains).  Samples do not change: chains are independent and their randomness is keyed
// by the chain's index in the caller's order (IterParams::orig).
static int run_sorted_phase(rmhmc_ctx* ctx, const Run& run, const IterBase& ib, const std::vector<long long>& T /* descending */, long long* progress_next) {
  const int n = (int)ctx->n;
  const long long Tmin = T[n - 1], Tmax = T[0];
  const bool ticking = progress_ticking(ctx);
  const long long chunk = ticking ? std::max<long long>(8, ctx->progress_every * (run.L + 1) / 2) : Tmax + 1;
  int done = 0;
  long long mi = 0;
  {
    StepGraph sg;
    if (step_graph_usable(ctx, run, std::min(Tmin, chunk))) (void)build_step_graph(ctx, run, ib, sg);
    for (long long left = Tmin; left > 0;) {
      const long long k = std::min(left, chunk);
      run_generic_steps(ctx, run, ib, k, &sg);
      left -= k;
      if (ticking) { RC(poll_progress(ctx, &done, &mi)); RC(progress_fire(ctx, progress_next, mi)); }
    }
    HIPCK(hipStreamSynchronize(ctx->stream));  // (the graph goes out of scope)
  }
  int na = n;
  for (long long s = Tmin; s < Tmax; ++s) {
    while (na > 0 && T[na - 1] <= s) --na;  // chains with T > s are still running: positions [0, na)
    const int nar = std::min(n, (na + 127) / 128 * 128);
    if (nar == n) launch_global_step(ctx, run, ctx->batch, ib);
    else launch_global_step_prefix(ctx, run, ib, nar);
    flow_tick(ctx);
    if (ticking && (s - Tmin) % chunk == chunk - 1) { RC(poll_progress(ctx, &done, &mi)); RC(progress_fire(ctx, progress_next, mi)); }
  }
  RC(poll_progress(ctx, &done, &mi));
  RC(progress_fire(ctx, progress_next, mi));
  if (done < n) RC(run_until_done(ctx, run, ib, 1, progress_next));  // (safety net: never taken if the schedule above is right)
  return RMHMC_OK;
}

}  // extern "C"

// ---- the write-out of a sampling call: to host or device memory, raw or reduced (include/rmhmc_out.h, output.hip.h) ------------------
// Every sampler has one body (sample_body, hmc_sample_body, ...) behind its two C entry points: the sampler's argument check, the
// statistics limit, the sample_to frame below and the counters.  <name>_sample_to checks its descriptor (out_check) and calls the body;
// the older <name>_sample[_dev|_stats|_stats_dev] checks what only it requires and calls the body with a descriptor of its own.  `who`
// is the entry point that was called, for the error text.
namespace {

// ESS / posterior summaries on the device (tools.py:32-74)
// the series length the kernel holds: checked by rmhmc_ess and rmhmc_ess_dev before they size or touch anything by S, and by every launch
int ess_range(rmhmc_ctx* ctx, long long S) {
  if (S < 2 || S > 20000) return fail(ctx, RMHMC_ERR_UNSUPPORTED, "ess: 2 <= S <= 20000 samples per chain (the centred series is held in LDS)");
  return RMHMC_OK;
}
int launch_ess(rmhmc_ctx* ctx, const double* d_samples, long long nblocks, long long S, int P, double* d_ess, double* d_mean, double* d_var) {
  RC(ess_range(ctx, S));
  HIPCK(hipFuncSetAttribute((const void*)k_ess, hipFuncAttributeMaxDynamicSharedMemorySize, MAX_LDS));  // per device: set where it is used
  long long nfft = 0;
  if (ctx->flags & RMHMC_FLAG_ESS_WRAP) { nfft = 1; while (nfft < S) nfft *= 2; nfft += 1; }  // tools.py:16-23
  hipLaunchKernelGGL(k_ess, dim3((unsigned)(nblocks * P)), dim3(64), (size_t)S * sizeof(double), ctx->stream, d_samples, S, P, d_ess, d_mean, d_var, nfft);
  return RMHMC_OK;
}

hipMemcpyKind out_kind(const rmhmc_out& out) { return out.where == RMHMC_OUT_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost; }
bool out_stats(const rmhmc_out& out) { return out.mean || out.var || out.ess || out.run_mean || out.run_ess; }

// the refusals of a caller's descriptor (the *_sample_to entry points only: the older ones build theirs, and rmhmc_sample_stats may
// ask for nothing but the counters)
int out_check(rmhmc_ctx* ctx, const char* who, const rmhmc_out* out) {
  if (!out) return fail(ctx, RMHMC_ERR_INVALID, std::string(who) + ": NULL output descriptor");
  if (out->where != RMHMC_OUT_HOST && out->where != RMHMC_OUT_DEVICE)
    return fail(ctx, RMHMC_ERR_INVALID, std::string(who) + ": where must be RMHMC_OUT_HOST or RMHMC_OUT_DEVICE");
  if (!out->samples && !out_stats(*out)) return fail(ctx, RMHMC_ERR_INVALID, std::string(who) + ": the output descriptor requests no output");
  return RMHMC_OK;
}

// The statistics limit, in every body after its argument check and before any sampling work.  A descriptor without raw samples is a
// statistics call even where every statistic is NULL (legal for rmhmc_sample_stats[_dev]): the limit holds for it all the same.
int stats_limit(rmhmc_ctx* ctx, const char* who, const rmhmc_out& out, int64_t S) {
  if ((!out.samples || out_stats(out)) && (S < 2 || S > 20000))
    return fail(ctx, RMHMC_ERR_UNSUPPORTED, std::string(who) + ": statistics need 2 <= n_iter - burn_in <= 20000 (the ESS kernel holds one series in LDS)");
  return RMHMC_OK;
}

// The write-out of a call: d_samples [n][S][D] in device memory -> whatever `out` requests, copied or reduced.  Returns with the
// stream idle and its own buffers freed.  Its wall time (the sampler has synchronised: the stream holds the counter copies at most) is
// kept for rmhmc_kernel_time "write_out".
int write_out(rmhmc_ctx* ctx, const double* d_samples, size_t n, size_t S, size_t D, const rmhmc_out& out) {
  const auto t0 = std::chrono::steady_clock::now();
  const hipMemcpyKind kind = out_kind(out);
  const size_t nd = n * D, sd = S * D;
  CallMem mem(ctx);
  const int rc = [&]() -> int {  // (a lambda: the time below is taken on every path, before mem frees)
    if (out.samples && out.samples != d_samples) HIPCK(hipMemcpyAsync(out.samples, d_samples, sizeof(double) * n * sd, kind, ctx->stream));
    if (out.mean || out.var || out.ess) {
      double* d_st = nullptr;  // [3][n][D]: ess, mean, var
      RC(mem.alloc(&d_st, sizeof(double) * 3 * nd));
      RC(launch_ess(ctx, d_samples, (long long)n, (long long)S, (int)D, d_st, d_st + nd, d_st + 2 * nd));
      if (out.ess) HIPCK(hipMemcpyAsync(out.ess, d_st, sizeof(double) * nd, kind, ctx->stream));
      if (out.mean) HIPCK(hipMemcpyAsync(out.mean, d_st + nd, sizeof(double) * nd, kind, ctx->stream));
      if (out.var) HIPCK(hipMemcpyAsync(out.var, d_st + 2 * nd, sizeof(double) * nd, kind, ctx->stream));
    }
    if (out.run_mean || out.run_ess) {
      double* d_rm = nullptr;  // [S][D] run mean, then [D] its ess
      RC(mem.alloc(&d_rm, sizeof(double) * (sd + D)));
      hipLaunchKernelGGL(k_run_mean, dim3((unsigned)((sd + 255) / 256)), dim3(256), 0, ctx->stream, d_samples, n, sd, d_rm);
      if (out.run_ess) RC(launch_ess(ctx, d_rm, 1, (long long)S, (int)D, d_rm + sd, nullptr, nullptr));
      if (out.run_mean) HIPCK(hipMemcpyAsync(out.run_mean, d_rm, sizeof(double) * sd, kind, ctx->stream));
      if (out.run_ess) HIPCK(hipMemcpyAsync(out.run_ess, d_rm + sd, sizeof(double) * D, kind, ctx->stream));
    }
    return sync(ctx);
  }();
  ctx->write_out_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

// a per-chain counter to the memory space of the descriptor (dst may be NULL)
template <typename T>
int counter_out(rmhmc_ctx* ctx, const rmhmc_out& out, int64_t* dst, const T* src) {
  static_assert(sizeof(T) == sizeof(int64_t), "int64");
  if (dst) HIPCK(hipMemcpyAsync(dst, src, sizeof(int64_t) * ctx->n, out_kind(out), ctx->stream));
  return RMHMC_OK;
}

// One sampling call after its checks.  core(d_samples) runs the sampler into d_samples [n][S][D] and queues its counter copies; the
// samples go straight into the caller's buffer where that is device memory, into a buffer of the call's otherwise.
template <typename F>
int sample_to(rmhmc_ctx* ctx, int64_t S, const rmhmc_out& out, F&& core) {
  const size_t n = ctx->n, D = ctx->D;
  const bool direct = out.where == RMHMC_OUT_DEVICE && out.samples;
  CallMem mem(ctx);
  double* d_samples = direct ? out.samples : nullptr;
  if (!direct) RC(mem.alloc(&d_samples, sizeof(double) * n * (size_t)S * D));
  RC(core(d_samples));
  return write_out(ctx, d_samples, n, (size_t)S, D, out);
}

}  // namespace

extern "C" {

// Runs the RMHMC sampler; the saved states go to the device buffer d_samples ([n][S][D], caller-provided).  *accepted and *steps say
// where the run left its per-chain counters, on the device in the caller's order: accepted proposals and post-burn-in leapfrog
// steps.  asked: the call's parameters in the caller's order (orig == nullptr); a work-sorted run steps with a copy that carries the map.
static int sample_core(rmhmc_ctx* ctx, const Run& asked, int64_t n_iter, int64_t burn_in, const double* theta0, double* d_samples, double* seconds_out,
                       const long long** accepted, const long long** steps) {
  const long long S = n_iter - burn_in;
  const int n = (int)ctx->n;
  // work-sorted layout (see run_sorted_phase): generic and one-launch stepping paths
  std::vector<long long> T;
  std::vector<double> th_perm;
  const bool sorted = !ctx->fused && n >= 2 && n_iter > burn_in + 1 && ctx->opt.sorted;
  long long progress_next = ctx->progress_first;
  if (sorted) {
    hipLaunchKernelGGL(k_traj_steps, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, (unsigned long long)asked.seed,
                       (long long)asked.chain_offset, asked.L, (long long)burn_in + 1, (long long)n_iter, (size_t)n, ctx->d_T);
    std::vector<long long> t0(n);
    RC(download(ctx, t0.data(), ctx->d_T, (size_t)n));
    RC(sync(ctx));
    std::vector<int> orig(n);
    for (int i = 0; i < n; ++i) orig[i] = i;
    std::stable_sort(orig.begin(), orig.end(), [&](int a, int b) { return t0[a] > t0[b]; });
    T.resize(n);
    for (int i = 0; i < n; ++i) T[i] = t0[orig[i]];
    RC(upload(ctx, ctx->d_orig, orig.data(), (size_t)n));
    RC(sync(ctx));
    th_perm.resize((size_t)n * ctx->D);
    for (int i = 0; i < n; ++i)
      for (int d = 0; d < ctx->D; ++d) th_perm[(size_t)i * ctx->D + d] = theta0 ? theta0[(size_t)orig[i] * ctx->D + d] : 1e-3;  // rmhmc.py:27
    theta0 = th_perm.data();
  }
  Run run = asked;
  if (sorted) run.orig = ctx->d_orig;
  RC(init_chains(ctx, theta0));
  // phase A: every chain completes transitions 0..burn_in; chains that get there first wait, so that
  // the timed phase B covers exactly the post-burn-in transitions (TimeTaken, rmhmc.py:194-198)
  const IterBase ipA{burn_in + 1, burn_in, S, d_samples, false, true};
  RC(run_phase(ctx, run, ipA, 0, &progress_next));
  HIPCK(hipMemcpyAsync(ctx->d_steps0, ctx->batch.ch.steps_done, sizeof(long long) * ctx->n, hipMemcpyDeviceToDevice, ctx->stream));
  HIPCK(hipMemsetAsync(ctx->d_done, 0, sizeof(int), ctx->stream));
  RC(sync(ctx));
  if (ctx->progress_fn) RC(report_progress(ctx, RMHMC_EV_BURNIN_DONE, burn_in + 1));  // rmhmc.py:194-196: banner, then the timer starts
  const auto t0 = std::chrono::steady_clock::now();
  if (n_iter > burn_in + 1) {
    const IterBase ipB{n_iter, burn_in, S, d_samples, false, true};
    if (sorted) RC(run_sorted_phase(ctx, run, ipB, T, &progress_next));
    else RC(run_phase(ctx, run, ipB, burn_in + 1, &progress_next, true));
  }
  RC(sync(ctx));
  if (seconds_out) *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  hipLaunchKernelGGL(k_sub_ll, dim3((unsigned)((ctx->n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->d_steps0, ctx->batch.ch.steps_done, (size_t)ctx->n);
  *accepted = ctx->batch.ch.accepted; *steps = ctx->d_steps0;
  if (sorted) {  // counters back into the caller's order: d_T[0..n) accepted, d_T[n..2n) post-burn-in steps
    const dim3 grid((unsigned)((n + 255) / 256));
    hipLaunchKernelGGL(k_scatter_ll, grid, dim3(256), 0, ctx->stream, ctx->d_T, ctx->batch.ch.accepted, ctx->d_orig, (size_t)n);
    hipLaunchKernelGGL(k_scatter_ll, grid, dim3(256), 0, ctx->stream, ctx->d_T + n, ctx->d_steps0, ctx->d_orig, (size_t)n);
    *accepted = ctx->d_T; *steps = ctx->d_T + n;
  }
  return RMHMC_OK;
}

static int sample_body(rmhmc_ctx* ctx, const char* who, int64_t n_iter, int64_t burn_in, int32_t L, double eps, int32_t K, uint64_t seed,
                       int64_t chain_offset, const double* theta0, const rmhmc_out& out, int64_t* accept_out, int64_t* steps_out,
                       double* seconds_out) {
  if (burn_in < 0 || burn_in >= n_iter || L < 1 || K < 1)
    return fail(ctx, RMHMC_ERR_INVALID, std::string(who) + ": need 0 <= burn_in < n_iter, L >= 1, K >= 1");
  RC(stats_limit(ctx, who, out, n_iter - burn_in));
  ctx->chains_ready = false;
  const Run run{RMHMC, L, K, eps, seed, chain_offset, nullptr};
  return sample_to(ctx, n_iter - burn_in, out, [&](double* d_samples) -> int {
    const long long *accepted = nullptr, *steps = nullptr;
    RC(sample_core(ctx, run, n_iter, burn_in, theta0, d_samples, seconds_out, &accepted, &steps));
    RC(counter_out(ctx, out, accept_out, accepted));
    return counter_out(ctx, out, steps_out, steps);
  });
}

int rmhmc_sample(rmhmc_ctx* ctx, int64_t n_iter, int64_t burn_in, int32_t L, double eps, int32_t K, uint64_t seed,
                 int64_t chain_offset, const double* theta0, double* samples_out, int64_t* accept_out, int64_t* steps_out,
                 double* seconds_out) {
  NEED_DATA(ctx);
  if (!samples_out) return fail(ctx, RMHMC_ERR_INVALID, "sample: need samples_out");
  return sample_body(ctx, "sample", n_iter, burn_in, L, eps, K, seed, chain_offset, theta0, {RMHMC_OUT_HOST, samples_out}, accept_out,
                     steps_out, seconds_out);
}
// (the sampler saves straight into the caller's HBM buffer: sample_to)
int rmhmc_sample_dev(rmhmc_ctx* ctx, int64_t n_iter, int64_t burn_in, int32_t L, double eps, int32_t K, uint64_t seed,
                     int64_t chain_offset, const double* theta0, double* samples_dev, int64_t* accept_dev, int64_t* steps_dev,
                     double* seconds_out) {
  NEED_DATA(ctx);
  if (!samples_dev) return fail(ctx, RMHMC_ERR_INVALID, "sample_dev: need samples_dev");
  return sample_body(ctx, "sample_dev", n_iter, burn_in, L, eps, K, seed, chain_offset, theta0, {RMHMC_OUT_DEVICE, samples_dev}, accept_dev,
                     steps_dev, seconds_out);
}
// (all three statistics may be NULL: the descriptor then asks for nothing, and the call returns the counters and the time)
int rmhmc_sample_stats(rmhmc_ctx* ctx, int64_t n_iter, int64_t burn_in, int32_t L, double eps, int32_t K, uint64_t seed,
                       int64_t chain_offset, const double* theta0, double* mean_out, double* var_out, double* ess_out,
                       int64_t* accept_out, int64_t* steps_out, double* seconds_out) {
  NEED_DATA(ctx);
  return sample_body(ctx, "sample_stats", n_iter, burn_in, L, eps, K, seed, chain_offset, theta0,
                     {RMHMC_OUT_HOST, nullptr, mean_out, var_out, ess_out}, accept_out, steps_out, seconds_out);
}
int rmhmc_sample_stats_dev(rmhmc_ctx* ctx, int64_t n_iter, int64_t burn_in, int32_t L, double eps, int32_t K, uint64_t seed,
                           int64_t chain_offset, const double* theta0, double* mean_dev, double* var_dev, double* ess_dev,
                           int64_t* accept_dev, int64_t* steps_dev, double* seconds_out) {
  NEED_DATA(ctx);
  return sample_body(ctx, "sample_stats_dev", n_iter, burn_in, L, eps, K, seed, chain_offset, theta0,
                     {RMHMC_OUT_DEVICE, nullptr, mean_dev, var_dev, ess_dev}, accept_dev, steps_dev, seconds_out);
}
int rmhmc_sample_to(rmhmc_ctx* ctx, int64_t n_iter, int64_t burn_in, int32_t L, double eps, int32_t K, uint64_t seed, int64_t chain_offset,
                    const double* theta0, const rmhmc_out* out, int64_t* accept_out, int64_t* steps_out, double* seconds_out) {
  NEED_DATA(ctx);
  RC(out_check(ctx, "sample_to", out));
  return sample_body(ctx, "sample_to", n_iter, burn_in, L, eps, K, seed, chain_offset, theta0, *out, accept_out, steps_out, seconds_out);
}

// ---- ESS of given samples (tools.py:32-74; launch_ess above) -------------------------------------------
int rmhmc_ess(rmhmc_ctx* ctx, const double* samples, int64_t n, int64_t S, int32_t P, double* ess_out) {
  if (!ctx || !samples || !ess_out || n < 1 || P < 1 || n * (int64_t)P > 0x7fffffffLL) return fail(ctx, RMHMC_ERR_INVALID, "ess: bad argument");
  RC(ess_range(ctx, S));  // before the buffers below are sized by S
  HIPCK(hipSetDevice(ctx->device));
  CallMem mem(ctx);
  double *d_s = nullptr, *d_e = nullptr;
  RC(mem.alloc(&d_s, sizeof(double) * (size_t)n * S * P));
  RC(mem.alloc(&d_e, sizeof(double) * (size_t)n * P));
  HIPCK(hipMemcpyAsync(d_s, samples, sizeof(double) * (size_t)n * S * P, hipMemcpyHostToDevice, ctx->stream));
  RC(launch_ess(ctx, d_s, n, S, P, d_e, nullptr, nullptr));
  HIPCK(hipMemcpyAsync(ess_out, d_e, sizeof(double) * (size_t)n * P, hipMemcpyDeviceToHost, ctx->stream));
  return sync(ctx);
}

int rmhmc_ess_dev(rmhmc_ctx* ctx, const double* samples_dev, int64_t n, int64_t S, int32_t P, double* ess_dev, double* mean_dev, double* var_dev) {
  if (!ctx || !samples_dev || (!ess_dev && !mean_dev && !var_dev) || n < 1 || P < 1 || n * (int64_t)P > 0x7fffffffLL)
    return fail(ctx, RMHMC_ERR_INVALID, "ess_dev: bad argument");
  RC(ess_range(ctx, S));
  HIPCK(hipSetDevice(ctx->device));
  RC(launch_ess(ctx, samples_dev, n, S, P, ess_dev, mean_dev, var_dev));
  return sync(ctx);
}

// ---- plain HMC (code/hmc.py) -------------------------------------------------------------------------
// evaluate gradient and log joint at theta0 and commit them as the current point of every chain (no run parameters, as init_chains);
// allow_traj = false: by the generic launches whatever the context (fixed-metric HMC never uses the one-launch trajectory kernel)
static int hmc_init_chains(rmhmc_ctx* ctx, const double* theta0_host /* [n][D] or NULL: zeros, hmc.py:27 */, bool allow_traj) {
  std::vector<double> th;
  if (!theta0_host) { th.assign((size_t)ctx->n * ctx->D, 0.0); theta0_host = th.data(); }
  RC(upload_vec(ctx, ctx->batch.ch.trj.w, theta0_host));
  fill_int(ctx, ctx->batch.ch.phase, 1, ctx->n);
  Group& g = ctx->batch;
  if (allow_traj && ctx->hmc_traj) {
    launch_hmc_traj(ctx, g, nullptr);
  } else {
    launch_rowpass<RP_G>(ctx, g, g.ch.trj.w, nullptr);
    SMALL(ctx, g, "small", k_hmc_init, ctx->dd, g.ch, ctx->nsplit);
  }
  return reset_chains(ctx);
}

// the per-chain buffers of the tempered sampler and of annealed importance sampling, on first use
static int ais_buffers(rmhmc_ctx* ctx) {
  if (ctx->d_ais_logw) return RMHMC_OK;
  if (!ctx->d_ais_ll) RC(dalloc(ctx, &ctx->d_ais_ll, ctx->n));
  if (!ctx->d_ais_ll0) RC(dalloc(ctx, &ctx->d_ais_ll0, ctx->n));
  return dalloc(ctx, &ctx->d_ais_logw, ctx->n);
}
// hmc_init_chains on the tempered target (include/rmhmc_ais.h), from the positions that are in trj.w already: the gradient pass and
// k_tphmc_init, which leaves loglik in d_ais_ll and d_ais_ll0 and, with logw, adds dbeta loglik to it (a stage of rmhmc_ais_run)
static int tphmc_init_dev(rmhmc_ctx* ctx, double beta, double* logw, double dbeta) {
  Group& g = ctx->batch;
  fill_int(ctx, g.ch.phase, 1, ctx->n);
  launch_rowpass<RP_G>(ctx, g, g.ch.trj.w, nullptr);
  launch(ctx, "ais", [&](hipStream_t st) {
    hipLaunchKernelGGL(k_tphmc_init, dim3((unsigned)g.n), dim3(64), 0, st, ctx->dd, g.ch, ctx->nsplit, beta, ctx->d_ais_ll, ctx->d_ais_ll0, logw, dbeta);
  });
  return reset_chains(ctx);
}
static int tphmc_init_chains(rmhmc_ctx* ctx, const double* theta0_host /* [n][D] or NULL: zeros */, double beta) {
  std::vector<double> th;
  if (!theta0_host) { th.assign((size_t)ctx->n * ctx->D, 0.0); theta0_host = th.data(); }
  RC(upload_vec(ctx, ctx->batch.ch.trj.w, theta0_host));
  return tphmc_init_dev(ctx, beta, nullptr, 0.0);  // (synchronises: the staging vector goes out of scope)
}

// one transition with the caller's randomness, plain (HMC), with the context's mass matrix (PHMC), or that on the target tempered by beta
// (TPHMC, which also returns loglik at the start and at the returned w)
static int hmc_transition_body(rmhmc_ctx* ctx, Sampler sampler, double* w, const double* z, const double* u_len, const double* u_acc, int32_t L,
                               double eps, int32_t* accepted_out, int32_t* nsteps_out, double* H_cur_out, double* H_prop_out,
                               double* w_prop_out, double* p_prop_out, int32_t* status_out, double beta = 1.0, double* loglik0_out = nullptr,
                               double* loglik_out = nullptr) {
  ctx->chains_ready = false;
  Run run{sampler, L, 0, eps, 0, 0, nullptr};  // (no fixed-point iterations: no K; the randomness is the caller's: no seed)
  run.beta = beta;
  if (sampler == TPHMC) {
    RC(ais_buffers(ctx));
    RC(tphmc_init_chains(ctx, w, beta));
    if (loglik0_out) RC(download(ctx, loglik0_out, ctx->d_ais_ll0, ctx->n));
  } else {
    RC(hmc_init_chains(ctx, w, sampler == HMC));
  }
  RC(upload(ctx, ctx->d_z, z, (size_t)ctx->n * ctx->D));
  RC(upload(ctx, ctx->d_ulen, u_len, ctx->n));
  RC(upload(ctx, ctx->d_uacc, u_acc, ctx->n));
  const IterBase ib{1, 0, 0, nullptr, true, false};
  for (int s = 0; s < L; ++s) launch_global_step(ctx, run, ctx->batch, ib);
  if (loglik_out && sampler == TPHMC) RC(download(ctx, loglik_out, ctx->d_ais_ll, ctx->n));
  return transition_out(ctx, w, accepted_out, nsteps_out, H_cur_out, H_prop_out, w_prop_out, p_prop_out, status_out);
}

int rmhmc_hmc_transition(rmhmc_ctx* ctx, double* w, const double* z, const double* u_len, const double* u_acc, int32_t L, double eps,
                         int32_t* accepted_out, int32_t* nsteps_out, double* H_cur_out, double* H_prop_out, double* w_prop_out,
                         double* p_prop_out) {
  NEED_DATA(ctx);
  if (!w || !z || !u_len || !u_acc || L < 1) return fail(ctx, RMHMC_ERR_INVALID, "hmc_transition: null pointer or L < 1");
  return hmc_transition_body(ctx, HMC, w, z, u_len, u_acc, L, eps, accepted_out, nsteps_out, H_cur_out, H_prop_out, w_prop_out, p_prop_out, nullptr);
}

// Runs the HMC sampler run.sampler names (HMC or PHMC); the saved states go to the device buffer d_samples ([n][S][D]).  It leaves the
// accepted proposals in batch.ch.accepted and, as sample_core, the post-burn-in leapfrog steps in d_steps0.
static int hmc_sample_run(rmhmc_ctx* ctx, const Run& run, int64_t n_iter, int64_t burn_in, double* d_samples, double* seconds_out);
static int hmc_sample_core(rmhmc_ctx* ctx, const Run& run, int64_t n_iter, int64_t burn_in, const double* theta0, double* d_samples, double* seconds_out) {
  RC(hmc_init_chains(ctx, theta0, run.sampler == HMC));
  return hmc_sample_run(ctx, run, n_iter, burn_in, d_samples, seconds_out);
}
// ... from chains that have their initial record (hmc_init_chains, or tphmc_init_chains for the tempered sampler)
static int hmc_sample_run(rmhmc_ctx* ctx, const Run& run, int64_t n_iter, int64_t burn_in, double* d_samples, double* seconds_out) {
  const long long S = n_iter - burn_in;
  long long progress_next = ctx->progress_first;
  const IterBase ipA{burn_in + 1, burn_in, S, d_samples, false, true};
  RC(run_phase(ctx, run, ipA, 0, &progress_next, false, true));
  HIPCK(hipMemcpyAsync(ctx->d_steps0, ctx->batch.ch.steps_done, sizeof(long long) * ctx->n, hipMemcpyDeviceToDevice, ctx->stream));
  HIPCK(hipMemsetAsync(ctx->d_done, 0, sizeof(int), ctx->stream));
  RC(sync(ctx));
  if (ctx->progress_fn) RC(report_progress(ctx, RMHMC_EV_BURNIN_DONE, burn_in + 1));  // hmc.py:92-94
  const auto t0 = std::chrono::steady_clock::now();
  if (n_iter > burn_in + 1) {
    // hmc.py:83-89 reports during burn-in only (`elif` of the save branch): no milestones, hence no cuts, inside TimeTaken
    const IterBase ipB{n_iter, burn_in, S, d_samples, false, true};
    RC(run_phase(ctx, run, ipB, burn_in + 1, nullptr));
  }
  RC(sync(ctx));
  if (seconds_out) *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  hipLaunchKernelGGL(k_sub_ll, dim3((unsigned)((ctx->n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->d_steps0, ctx->batch.ch.steps_done, (size_t)ctx->n);
  return RMHMC_OK;
}

static int hmc_sample_body(rmhmc_ctx* ctx, const char* who, int64_t n_iter, int64_t burn_in, int32_t L, double eps, uint64_t seed,
                           int64_t chain_offset, const double* theta0, const rmhmc_out& out, int64_t* accept_out, int64_t* steps_out,
                           double* seconds_out) {
  if (burn_in < 0 || burn_in >= n_iter || L < 1) return fail(ctx, RMHMC_ERR_INVALID, std::string(who) + ": need 0 <= burn_in < n_iter, L >= 1");
  RC(stats_limit(ctx, who, out, n_iter - burn_in));
  ctx->chains_ready = false;
  const Run run{HMC, L, 0, eps, seed, chain_offset, nullptr};  // (no fixed-point iterations: no K)
  return sample_to(ctx, n_iter - burn_in, out, [&](double* d_samples) -> int {
    RC(hmc_sample_core(ctx, run, n_iter, burn_in, theta0, d_samples, seconds_out));
    RC(counter_out(ctx, out, accept_out, ctx->batch.ch.accepted));
    return counter_out(ctx, out, steps_out, ctx->d_steps0);
  });
}

int rmhmc_hmc_sample(rmhmc_ctx* ctx, int64_t n_iter, int64_t burn_in, int32_t L, double eps, uint64_t seed, int64_t chain_offset,
                     const double* theta0, double* samples_out, int64_t* accept_out, int64_t* steps_out, double* seconds_out) {
  NEED_DATA(ctx);
  if (!samples_out) return fail(ctx, RMHMC_ERR_INVALID, "hmc_sample: need samples_out");
  return hmc_sample_body(ctx, "hmc_sample", n_iter, burn_in, L, eps, seed, chain_offset, theta0, {RMHMC_OUT_HOST, samples_out}, accept_out,
                         steps_out, seconds_out);
}
int rmhmc_hmc_sample_to(rmhmc_ctx* ctx, int64_t n_iter, int64_t burn_in, int32_t L, double eps, uint64_t seed, int64_t chain_offset,
                        const double* theta0, const rmhmc_out* out, int64_t* accept_out, int64_t* steps_out, double* seconds_out) {
  NEED_DATA(ctx);
  RC(out_check(ctx, "hmc_sample_to", out));
  return hmc_sample_body(ctx, "hmc_sample_to", n_iter, burn_in, L, eps, seed, chain_offset, theta0, *out, accept_out, steps_out, seconds_out);
}

// ---- HMC with a fixed dense mass matrix shared by all chains (include/rmhmc_phmc.h, phmc.hip.h, mass.h) ----------------
// the two images of a mass matrix (mass.h) into the context
static int install_mass_images(rmhmc_ctx* ctx, const std::vector<double>& Lm, const std::vector<double>& Mi) {
  const size_t nn = (size_t)ctx->DP * ctx->DP;
  if (!ctx->d_massInv) {  // first use: the LDS limit of this shape's kernels (more than 64 KB for DP > 128), and the images
    // (what the instantiation needs, the same for every context that uses it - not MAX_LDS: the kernels have static LDS besides)
    int rc = RMHMC_OK;
    PHMC_SWITCH(ctx, rc = raise_lds(ctx, k_phmc_head<NDB_>, (int)phmc_lds_bytes<NDB_>());
                if (rc == RMHMC_OK) rc = raise_lds(ctx, k_phmc_tail<NDB_>, (int)phmc_lds_bytes<NDB_>());
                if (rc == RMHMC_OK) rc = raise_lds(ctx, k_tphmc_tail<NDB_>, (int)phmc_lds_bytes<NDB_>()));
    RC(rc);
    if (!ctx->d_massL) RC(dalloc(ctx, &ctx->d_massL, nn));
    RC(dalloc(ctx, &ctx->d_massInv, nn));
  }
  RC(upload(ctx, ctx->d_massL, Lm.data(), nn));
  RC(upload(ctx, ctx->d_massInv, Mi.data(), nn));
  RC(sync(ctx));  // (the caller's staging vectors may go out of scope)
  ctx->have_mass = true;
  return RMHMC_OK;
}
int rmhmc_phmc_set_mass(rmhmc_ctx* ctx, const double* mass) {
  if (!ctx) return fail(nullptr, RMHMC_ERR_INVALID, "null context");
  HIPCK(hipSetDevice(ctx->device));
  std::vector<double> Lm, Mi;
  const char* why = "";
  if (mass_images(mass, ctx->D, ctx->DP, Lm, Mi, &why) != RMHMC_OK) return fail(ctx, RMHMC_ERR_INVALID, std::string("phmc_set_mass: ") + why);
  return install_mass_images(ctx, Lm, Mi);
}

int rmhmc_phmc_mode(rmhmc_ctx* ctx, const double* w0, int32_t max_iter, double tol, double* w_out, double* G_out, int32_t* iters_out,
                    double* step_out) {
  NEED_DATA(ctx);
  if (!w_out || max_iter < 0 || !(tol >= 0.0)) return fail(ctx, RMHMC_ERR_INVALID, "phmc_mode: need w_out, max_iter >= 0, tol >= 0");
  ctx->chains_ready = false;
  Group& g = ctx->batch;
  const size_t n = ctx->n, D = ctx->D, DP = ctx->DP;
  if (ctx->big && !ctx->d_Gcopy) RC(dalloc(ctx, &ctx->d_Gcopy, n * DP * DP));
  std::vector<double> w(D, 0.0), s(D), W(n * D), ljl(n), G(G_out ? D * D : 0);
  if (w0) w.assign(w0, w0 + D);
  // The batch evaluates one point per chain: the Newton system at w on every chain (chain 0 is read), then the log joint of w and of
  // the candidates w + s / 2^k, k = 0..20, as many at a time as there are chains.
  constexpr int NPTS = 22;
  auto point = [&](int idx, size_t d) { return idx == 0 ? w[d] : w[d] + std::ldexp(s[d], -(idx - 1)); };
  int32_t it = 0;
  double step = 0.0;
  for (;; ++it) {
    for (size_t c = 0; c < n; ++c) std::copy(w.begin(), w.end(), W.begin() + c * D);
    RC(upload_vec(ctx, g.ch.trj.w, W.data()));
    HIPCK(hipMemsetAsync(g.ch.p, 0, sizeof(double) * n * DP, ctx->stream));
    fill_int(ctx, g.ch.phase, 1, n);
    fill_int(ctx, g.ch.status, 0, n);
    eval_point_phases(ctx, g, nullptr, 1, ctx->big);                               // G, its factor, G^-1, gradient, log joint
    SMALL(ctx, g, "small", k_ginv_matvec, ctx->D, ctx->DP, g.ch, g.ch.trj.grad);  // s = G^-1 grad -> uq
    RC(download(ctx, s.data(), g.ch.uq, D));
    if (G_out)
      HIPCK(hipMemcpy2DAsync(G.data(), D * 8, ctx->big ? ctx->d_Gcopy : g.ch.Gq, DP * 8, D * 8, D, hipMemcpyDeviceToHost, ctx->stream));
    RC(sync(ctx));
    double wmax = 0.0;
    step = 0.0;
    for (size_t d = 0; d < D; ++d) { step = std::fmax(step, std::fabs(s[d])); wmax = std::fmax(wmax, std::fabs(w[d])); if (s[d] != s[d]) step = s[d]; }
    if (!std::isfinite(step) || step <= tol * std::fmax(1.0, wmax) || it >= max_iter) break;
    bool taken = false;
    double base = 0.0;
    for (int first = 0; first < NPTS && !taken; first += (int)n) {
      for (size_t c = 0; c < n; ++c)
        for (size_t d = 0; d < D; ++d) W[c * D + d] = point(std::min(first + (int)c, NPTS - 1), d);
      RC(upload_vec(ctx, g.ch.trj.w, W.data()));
      fill_int(ctx, g.ch.phase, 1, n);
      launch_rowpass<RP_G>(ctx, g, g.ch.trj.w, nullptr);
      SMALL(ctx, g, "small", k_hmc_init, ctx->dd, g.ch, ctx->nsplit);
      RC(download(ctx, ljl.data(), g.ch.trj.ljl, n));
      RC(sync(ctx));
      for (int c = 0; c < (int)n && first + c < NPTS && !taken; ++c) {
        const int idx = first + c;
        if (idx == 0) { base = ljl[0]; continue; }
        if (std::isfinite(ljl[c]) && ljl[c] >= base) {
          for (size_t d = 0; d < D; ++d) w[d] = W[(size_t)c * D + d];
          taken = true;
        }
      }
    }
    if (!taken) break;
  }
  std::copy(w.begin(), w.end(), w_out);
  if (G_out) {
    std::copy(G.begin(), G.end(), G_out);
    if (ctx->i8)  // the int8 assembly writes the lower triangle only
      for (size_t a = 0; a < D; ++a)
        for (size_t b = a + 1; b < D; ++b) G_out[a * D + b] = G_out[b * D + a];
  }
  if (iters_out) *iters_out = it;
  if (step_out) *step_out = step;
  return RMHMC_OK;
}

int rmhmc_phmc_transition(rmhmc_ctx* ctx, double* w, const double* z, const double* u_len, const double* u_acc, int32_t L, double eps,
                          int32_t* accepted_out, int32_t* nsteps_out, double* H_cur_out, double* H_prop_out, double* w_prop_out,
                          double* p_prop_out, int32_t* status_out) {
  NEED_DATA(ctx);
  if (!w || !z || !u_len || !u_acc || L < 1) return fail(ctx, RMHMC_ERR_INVALID, "phmc_transition: null pointer or L < 1");
  if (!ctx->have_mass) return fail(ctx, RMHMC_ERR_INVALID, "phmc_transition: rmhmc_phmc_set_mass has not been called");
  return hmc_transition_body(ctx, PHMC, w, z, u_len, u_acc, L, eps, accepted_out, nsteps_out, H_cur_out, H_prop_out, w_prop_out, p_prop_out, status_out);
}

static int phmc_sample_body(rmhmc_ctx* ctx, const char* who, int64_t n_iter, int64_t burn_in, int32_t L, double eps, uint64_t seed,
                            int64_t chain_offset, const double* theta0, const rmhmc_out& out, int64_t* accept_out, int64_t* steps_out,
                            double* seconds_out) {
  if (burn_in < 0 || burn_in >= n_iter || L < 1) return fail(ctx, RMHMC_ERR_INVALID, std::string(who) + ": need 0 <= burn_in < n_iter, L >= 1");
  if (!ctx->have_mass) return fail(ctx, RMHMC_ERR_INVALID, std::string(who) + ": rmhmc_phmc_set_mass has not been called");
  RC(stats_limit(ctx, who, out, n_iter - burn_in));
  ctx->chains_ready = false;
  const Run run{PHMC, L, 0, eps, seed, chain_offset, nullptr};  // (no fixed-point iterations: no K)
  return sample_to(ctx, n_iter - burn_in, out, [&](double* d_samples) -> int {
    RC(hmc_sample_core(ctx, run, n_iter, burn_in, theta0, d_samples, seconds_out));
    RC(counter_out(ctx, out, accept_out, ctx->batch.ch.accepted));
    return counter_out(ctx, out, steps_out, ctx->d_steps0);
  });
}

int rmhmc_phmc_sample_to(rmhmc_ctx* ctx, int64_t n_iter, int64_t burn_in, int32_t L, double eps, uint64_t seed, int64_t chain_offset,
                         const double* theta0, const rmhmc_out* out, int64_t* accept_out, int64_t* steps_out, double* seconds_out) {
  NEED_DATA(ctx);
  RC(out_check(ctx, "phmc_sample_to", out));
  return phmc_sample_body(ctx, "phmc_sample_to", n_iter, burn_in, L, eps, seed, chain_offset, theta0, *out, accept_out, steps_out, seconds_out);
}

// ---- simplified manifold MALA (BLR_mMALA_Simp.m) -------------------------------------------------------------
// (run: the step size, the Philox key and the sampler kind of the RMHMC records; mMALA has no L and no K)
static void launch_mmala_step(rmhmc_ctx* ctx, const Run& run, Group& g, const IterBase& b) {
  const double eps = run.eps;
  const int full = (ctx->flags & RMHMC_FLAG_MMALA_FULL) ? 1 : 0;
  const IterParams ip = iter_params(ctx, run, b);
  SMALL(ctx, g, "small", k_mmala_begin, ctx->D, ctx->DP, g.ch, ip, eps, full);
  eval_point_phases(ctx, g, nullptr, full ? 2 : 1);
  SMALL(ctx, g, "small", k_mmala_end, ctx->D, ctx->DP, g.ch, ip, eps, full);
}
// record at theta0: mMALA never uses the fused stepping kernel, so not by its evaluation either; by the one-launch step kernel's where
// the context has it, unless the caller (IWLS) wants the generic kernels throughout
static int mmala_init(rmhmc_ctx* ctx, const double* theta0_host, bool allow_medium = true) {
  std::vector<double> th;
  if (!theta0_host) { th.assign((size_t)ctx->n * ctx->D, 0.0); theta0_host = th.data(); }  // BLR_mMALA_Simp.m:175
  return init_chains(ctx, theta0_host, false, allow_medium);
}

int rmhmc_mmala_transition(rmhmc_ctx* ctx, double* w, const double* z, const double* u_acc, double eps, int32_t* accepted_out,
                           double* ratio_out, double* w_prop_out) {
  NEED_DATA(ctx);
  if (!w || !z || !u_acc || !(eps > 0)) return fail(ctx, RMHMC_ERR_INVALID, "mmala_transition: null pointer or eps <= 0");
  ctx->chains_ready = false;
  const Run run{RMHMC, 0, 0, eps, 0, 0, nullptr};
  RC(mmala_init(ctx, w));
  RC(upload(ctx, ctx->d_z, z, (size_t)ctx->n * ctx->D));
  RC(upload(ctx, ctx->d_uacc, u_acc, ctx->n));
  const IterBase ib{1, 0, 0, nullptr, true, false};
  launch_mmala_step(ctx, run, ctx->batch, ib);
  return transition_out(ctx, w, accepted_out, nullptr, nullptr, ratio_out /* Hprop */, w_prop_out, nullptr, nullptr);
}

// Runs the simplified mMALA sampler; the saved states go to the device buffer d_samples ([n][S][D]), the accepted proposals stay in
// batch.ch.accepted.
static int mmala_sample_core(rmhmc_ctx* ctx, const Run& run, int64_t n_iter, int64_t burn_in, const double* theta0, double* d_samples, double* seconds_out) {
  RC(mmala_init(ctx, theta0));
  const IterBase ib{n_iter, burn_in, n_iter - burn_in, d_samples, false, false};
  for (int64_t it = 0; it <= burn_in; ++it) { launch_mmala_step(ctx, run, ctx->batch, ib); flow_tick(ctx); }
  RC(sync(ctx));
  const auto t0 = std::chrono::steady_clock::now();
  for (int64_t it = burn_in + 1; it < n_iter; ++it) { launch_mmala_step(ctx, run, ctx->batch, ib); flow_tick(ctx); }
  RC(sync(ctx));
  if (seconds_out) *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return RMHMC_OK;
}

static int mmala_sample_body(rmhmc_ctx* ctx, const char* who, int64_t n_iter, int64_t burn_in, double eps, uint64_t seed, int64_t chain_offset,
                             const double* theta0, const rmhmc_out& out, int64_t* accept_out, double* seconds_out) {
  if (burn_in < 0 || burn_in >= n_iter || !(eps > 0)) return fail(ctx, RMHMC_ERR_INVALID, std::string(who) + ": need 0 <= burn_in < n_iter, eps > 0");
  RC(stats_limit(ctx, who, out, n_iter - burn_in));
  ctx->chains_ready = false;
  const Run run{RMHMC, 0, 0, eps, seed, chain_offset, nullptr};
  return sample_to(ctx, n_iter - burn_in, out, [&](double* d_samples) -> int {
    RC(mmala_sample_core(ctx, run, n_iter, burn_in, theta0, d_samples, seconds_out));
    return counter_out(ctx, out, accept_out, ctx->batch.ch.accepted);
  });
}

int rmhmc_mmala_sample(rmhmc_ctx* ctx, int64_t n_iter, int64_t burn_in, double eps, uint64_t seed, int64_t chain_offset,
                       const double* theta0, double* samples_out, int64_t* accept_out, double* seconds_out) {
  NEED_DATA(ctx);
  if (!samples_out) return fail(ctx, RMHMC_ERR_INVALID, "mmala_sample: need samples_out");
  return mmala_sample_body(ctx, "mmala_sample", n_iter, burn_in, eps, seed, chain_offset, theta0, {RMHMC_OUT_HOST, samples_out}, accept_out,
                           seconds_out);
}
int rmhmc_mmala_sample_to(rmhmc_ctx* ctx, int64_t n_iter, int64_t burn_in, double eps, uint64_t seed, int64_t chain_offset,
                          const double* theta0, const rmhmc_out* out, int64_t* accept_out, double* seconds_out) {
  NEED_DATA(ctx);
  RC(out_check(ctx, "mmala_sample_to", out));
  return mmala_sample_body(ctx, "mmala_sample_to", n_iter, burn_in, eps, seed, chain_offset, theta0, *out, accept_out, seconds_out);
}

int rmhmc_chains_init(rmhmc_ctx* ctx, const double* theta0, uint64_t seed, int64_t chain_offset, int32_t L, double eps, int32_t K) {
  NEED_DATA(ctx);
  if (L < 1 || K < 1) return fail(ctx, RMHMC_ERR_INVALID, "chains_init: L >= 1 and K >= 1 required");
  RC(init_chains(ctx, theta0));
  if (ctx->batch.dcount) HIPCK(hipMemsetAsync(ctx->batch.dcount, 0, 6 * sizeof(unsigned long long), ctx->stream));
  ctx->chains = Run{RMHMC, L, K, eps, seed, chain_offset, nullptr};
  ctx->chains_ready = true;
  return RMHMC_OK;
}

int rmhmc_chains_run(rmhmc_ctx* ctx, int64_t n_steps) {
  NEED_DATA(ctx);
  if (!ctx->chains_ready) return fail(ctx, RMHMC_ERR_INVALID, "chains_run: rmhmc_chains_init has not been called");
  const Run& run = ctx->chains;  // (chains_ready holds)
  const IterBase ib{(long long)1 << 62, 0, 0, nullptr, false, false};
  {
    Timed t(ctx, "total", ctx->stream);
    if (ctx->fused) {
      launch_fused(ctx, run, ib, n_steps);
    } else {
      StepGraph sg;
      if (step_graph_usable(ctx, run, n_steps)) (void)build_step_graph(ctx, run, ib, sg);
      run_generic_steps(ctx, run, ib, n_steps, &sg);
      HIPCK(hipStreamSynchronize(ctx->stream));  // the graph is destroyed at the end of this scope
    }
  }
  return sync(ctx);
}

static int chains_state_impl(rmhmc_ctx* ctx, double* w_out, int64_t* iters_out, int64_t* accept_out, bool dev) {
  NEED_DATA(ctx);
  if (!ctx->chains_ready) return fail(ctx, RMHMC_ERR_INVALID, "chains_state: rmhmc_chains_init has not been called");
  const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (w_out) RC(copy_rows(ctx, w_out, ctx->D, ctx->batch.ch.cur.w, ctx->DP, ctx->D, ctx->n, kind));  // strip the padding: [n][DP] -> [n][D]
  static_assert(sizeof(long long) == sizeof(int64_t), "int64");
  if (iters_out) HIPCK(hipMemcpyAsync(iters_out, ctx->batch.ch.iter, sizeof(int64_t) * ctx->n, kind, ctx->stream));
  if (accept_out) HIPCK(hipMemcpyAsync(accept_out, ctx->batch.ch.accepted, sizeof(int64_t) * ctx->n, kind, ctx->stream));
  return sync(ctx);
}
int rmhmc_chains_state(rmhmc_ctx* ctx, double* w_out, int64_t* iters_out, int64_t* accept_out) {
  return chains_state_impl(ctx, w_out, iters_out, accept_out, false);
}
int rmhmc_chains_state_dev(rmhmc_ctx* ctx, double* w_dev, int64_t* iters_dev, int64_t* accept_dev) {
  return chains_state_impl(ctx, w_dev, iters_dev, accept_dev, true);
}

int rmhmc_chains_restore(rmhmc_ctx* ctx, const int64_t* iters, const int64_t* accepted) {
  NEED_DATA(ctx);
  if (!ctx->chains_ready || !iters || !accepted) return fail(ctx, RMHMC_ERR_INVALID, "chains_restore: call rmhmc_chains_init first");
  for (int64_t c = 0; c < ctx->n; ++c)
    if (iters[c] < 0 || accepted[c] < 0) return fail(ctx, RMHMC_ERR_INVALID, "chains_restore: negative counter");
  RC(upload(ctx, ctx->batch.ch.iter, (const long long*)iters, ctx->n));
  RC(upload(ctx, ctx->batch.ch.accepted, (const long long*)accepted, ctx->n));
  return sync(ctx);
}

int rmhmc_set_progress(rmhmc_ctx* ctx, rmhmc_progress_fn fn, int64_t first, int64_t every, void* user) {
  if (!ctx || (fn && (first < 1 || every < 1))) return fail(ctx, RMHMC_ERR_INVALID, "set_progress: first >= 1 and every >= 1 required");
  ctx->progress_fn = fn; ctx->progress_first = first; ctx->progress_every = every; ctx->progress_user = user;
  return RMHMC_OK;
}

int rmhmc_int8_certificate(rmhmc_ctx* ctx, double* bound_out, int32_t* active_out) {
  if (!ctx) return fail(nullptr, RMHMC_ERR_INVALID, "int8_certificate: null context");
  if (bound_out) *bound_out = ctx->i8_bound;
  if (active_out) *active_out = (ctx->i8_requested && ctx->i8) ? 1 : 0;
  return RMHMC_OK;
}

int rmhmc_kernel_time(rmhmc_ctx* ctx, const char* which, double* seconds_out, int64_t* launches_out) {
  if (!ctx || !which) return fail(ctx, RMHMC_ERR_INVALID, "kernel_time: bad argument");
  HIPCK(hipSetDevice(ctx->device));
  const std::string w(which);
  if (seconds_out) *seconds_out = 0.0;
  if (launches_out) *launches_out = 0;
  if (w == "enable") { ctx->timing = true; return RMHMC_OK; }
  if (w == "disable") { ctx->timing = false; return RMHMC_OK; }
  if (w == "write_out") {  // (include/rmhmc_out.h)
    if (seconds_out) *seconds_out = ctx->write_out_seconds;
    if (launches_out) *launches_out = 1;
    return RMHMC_OK;
  }
  if (w == "reset") {
    RC(sync(ctx));
    for (auto& kv : ctx->events) { for (auto& e : kv.second) ctx->pool.push_back(e); kv.second.clear(); }
    return RMHMC_OK;
  }
  RC(sync(ctx));
  if (w.rfind("i8_delta_", 0) == 0) {  // delta assemblies by slice count (I8Delta::count): [3 (6 - seff) + S' - 4]
    static const char* const names[5] = {"i8_delta_end_s4", "i8_delta_end_s5", "i8_delta_end_s6", "i8_delta_inner_s4", "i8_delta_inner_s5"};
    const int slot = (int)(std::find_if(names, names + 5, [&](const char* s) { return w == s; }) - names);
    if (slot == 5) return fail(ctx, RMHMC_ERR_INVALID, "kernel_time: unknown delta counter " + w);
    if (ctx->batch.dcount) {
      unsigned long long h = 0;
      HIPCK(hipMemcpy(&h, ctx->batch.dcount + slot, sizeof(h), hipMemcpyDeviceToHost));
      if (launches_out) *launches_out = (int64_t)h;
    }
    return RMHMC_OK;
  }
  auto it = ctx->events.find(w);
  if (it == ctx->events.end()) return RMHMC_OK;
  double ms = 0.0;
  for (auto& e : it->second) {
    float m = 0.f;
    HIPCK(hipEventElapsedTime(&m, e.a, e.b));
    ms += m;
  }
  if (seconds_out) *seconds_out = ms * 1e-3;
  if (launches_out) *launches_out = (int64_t)it->second.size();
  return RMHMC_OK;
}

}  // extern "C"

// ---- adaptive Metropolis (metropolis.py, amh.hip.h) --------------------------------------------------------------------------------
namespace {

// Runs iterations 0..n_iter-1 of every chain in segments (metropolis.py:38-91), p carries the mode.  Progress reports and the timer
// sit between segments.  A segment ends after at most 1000 iterations, after every reported iteration and after iteration burn_in,
// the same cuts for any number of chains; its launches are cut by work (AMH_LAUNCH_ROWS), which leaves the results unchanged.
int amh_run(rmhmc_ctx* ctx, AmhParams p, const double* theta0, double* seconds_out) {
  const size_t n = ctx->n, D = ctx->D, DP = ctx->DP;
  Chains& ch = ctx->batch.ch;
  std::vector<double> h((size_t)n * D, 0.0);
  RC(upload_vec(ctx, ch.cur.w, theta0 ? theta0 : h.data()));
  std::fill(h.begin(), h.end(), 1.0);
  RC(upload_vec(ctx, ch.PM, h.data()));
  HIPCK(hipMemsetAsync(ch.u0, 0, sizeof(double) * n * DP, ctx->stream));
  fill_ll(ctx, ch.accepted, 0, n);
  p.w = ch.cur.w; p.sd = ch.PM; p.accw = ch.u0; p.ljl = ch.cur.ljl; p.accepted = ch.accepted; p.fa = ch.rv0; p.fb = ch.rv2;
  const AmhShape shape = amh_shape(ctx->M, ctx->n);  // (plan.h)
  const int NT = shape.nt, R = shape.rows;
  const bool sampling = p.z_in == nullptr;
  const long long N = p.n_iter, B = p.burn_in;
  auto t0 = std::chrono::steady_clock::now();
  for (long long start = 0; start < N;) {
    long long end = std::min(N, start + 1000);
    if (start <= B) {
      end = std::min(end, B + 1);
      const long long rep = (start + 999) / 1000 * 1000;  // next reported iteration >= start
      if (rep < B) end = std::min(end, rep + 1);
    }
    // the segment [start, end) in launches of at most AMH_LAUNCH_ROWS evaluations each; f is recomputed at the segment's start only
    const long long per_iter = (long long)n * (long long)D * ctx->M;
    const long long step = std::max(1LL, AMH_LAUNCH_ROWS / std::max(1LL, per_iter));
    for (long long a = start; a < end; a += step) {
      p.it0 = a; p.it1 = std::min(end, a + step); p.carry = a > start ? 1 : 0;
      AMH_SWITCH(NT, R, hipLaunchKernelGGL((k_amh<NT_, R_>), dim3((unsigned)n), dim3(NT_), 0, ctx->stream, ctx->dd, p));
      HIPCK(hipGetLastError());
    }
    const long long last = end - 1;
    if (sampling && last <= B) {
      RC(sync(ctx));
      if (ctx->progress_fn && last % 1000 == 0 && last < B) ctx->progress_fn(RMHMC_EV_PROGRESS, last, 0, 0, ctx->progress_user);
      if (last == B) {
        if (ctx->progress_fn) ctx->progress_fn(RMHMC_EV_BURNIN_DONE, B, 0, 0, ctx->progress_user);
        t0 = std::chrono::steady_clock::now();
      }
    }
    start = end;
  }
  RC(sync(ctx));
  if (seconds_out) *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return RMHMC_OK;
}

bool amh_iters_ok(int64_t n_iter, int64_t burn_in) { return burn_in >= 0 && burn_in < n_iter && n_iter <= (int64_t)0xffffffffLL; }

int amh_sample_body(rmhmc_ctx* ctx, const char* who, int64_t n_iter, int64_t burn_in, uint64_t seed, int64_t chain_offset, const double* theta0,
                    const rmhmc_out& out, int64_t* accepted_out, double* sd_out, double* seconds_out) {
  if (!amh_iters_ok(n_iter, burn_in) || chain_offset < 0)
    return fail(ctx, RMHMC_ERR_INVALID, std::string(who) + ": need 0 <= burn_in < n_iter < 2^32, chain_offset >= 0");
  RC(stats_limit(ctx, who, out, n_iter - burn_in));
  ctx->chains_ready = false;
  return sample_to(ctx, n_iter - burn_in, out, [&](double* d_samples) -> int {
    AmhParams p{};
    p.samples = d_samples; p.seed = seed; p.chain_offset = chain_offset; p.n_iter = n_iter; p.burn_in = burn_in;
    RC(amh_run(ctx, p, theta0, seconds_out));
    RC(counter_out(ctx, out, accepted_out, ctx->batch.ch.accepted));
    if (sd_out) RC(copy_rows(ctx, sd_out, ctx->D, ctx->batch.ch.PM, ctx->DP, ctx->D, ctx->n, out_kind(out)));  // [n][DP] -> [n][D]
    return RMHMC_OK;
  });
}

}  // namespace

extern "C" {

int rmhmc_amh_sample(rmhmc_ctx* ctx, int64_t n_iter, int64_t burn_in, uint64_t seed, int64_t chain_offset, const double* theta0,
                     double* samples_out, int64_t* accepted_out, double* sd_out, double* seconds_out) {
  NEED_DATA(ctx);
  if (!samples_out) return fail(ctx, RMHMC_ERR_INVALID, "amh_sample: need samples_out");
  return amh_sample_body(ctx, "amh_sample", n_iter, burn_in, seed, chain_offset, theta0, {RMHMC_OUT_HOST, samples_out}, accepted_out, sd_out,
                         seconds_out);
}
int rmhmc_amh_sample_to(rmhmc_ctx* ctx, int64_t n_iter, int64_t burn_in, uint64_t seed, int64_t chain_offset, const double* theta0,
                        const rmhmc_out* out, int64_t* accepted_out, double* sd_out, double* seconds_out) {
  NEED_DATA(ctx);
  RC(out_check(ctx, "amh_sample_to", out));
  return amh_sample_body(ctx, "amh_sample_to", n_iter, burn_in, seed, chain_offset, theta0, *out, accepted_out, sd_out, seconds_out);
}

int rmhmc_amh_replay(rmhmc_ctx* ctx, int64_t n_iter, int64_t burn_in, const double* z, const double* u, const double* theta0,
                     double* w_out, double* ljl_out, double* sd_out, int8_t* decisions_out) {
  NEED_DATA(ctx);
  if (!z || !u || !w_out || !ljl_out || !decisions_out || !amh_iters_ok(n_iter, burn_in))
    return fail(ctx, RMHMC_ERR_INVALID, "amh_replay: need z, u, w_out, ljl_out, decisions_out and 0 <= burn_in < n_iter < 2^32");
  ctx->chains_ready = false;
  const size_t n = ctx->n, D = ctx->D, T = (size_t)n_iter, vec = n * T * D;
  CallMem mem(ctx);
  double *d_z = nullptr, *d_u = nullptr, *d_w = nullptr, *d_l = nullptr;
  int8_t* d_dec = nullptr;
  RC(mem.alloc(&d_z, sizeof(double) * vec)); RC(mem.alloc(&d_u, sizeof(double) * vec));
  RC(mem.alloc(&d_w, sizeof(double) * vec)); RC(mem.alloc(&d_l, sizeof(double) * n * T));
  RC(mem.alloc(&d_dec, vec));
  RC(upload(ctx, d_z, z, vec)); RC(upload(ctx, d_u, u, vec));
  AmhParams p{};
  p.z_in = d_z; p.u_in = d_u; p.w_out = d_w; p.ljl_out = d_l; p.dec_out = d_dec; p.n_iter = n_iter; p.burn_in = burn_in;
  RC(amh_run(ctx, p, theta0, nullptr));
  RC(download(ctx, w_out, d_w, vec)); RC(download(ctx, ljl_out, d_l, n * T)); RC(download(ctx, decisions_out, d_dec, vec));
  if (sd_out) RC(download_vec(ctx, sd_out, ctx->batch.ch.PM));
  return sync(ctx);
}

}  // extern "C"

// ---- IWLS Metropolis-Hastings (iwls.py, iwls.hip.h) --------------------------------------------------------------------------------
namespace {

const char* const kIwlsDMsg = "iwls: D > 64 is not supported (64 < D <= 256 needs a blocked factorisation of G^-1 + 1e-6 I)";

// The iteration loop of IWLS and Gibbs.  Sampling: before iterations i % every == 0 and burn_in, report(i) does what the sampler's
// reference prints there (it synchronises if it has to); before iteration burn_in the stream is drained and the timer restarts.
// step(i) queues the launches of iteration i.
template <typename Report, typename Step>
int timed_iterations(rmhmc_ctx* ctx, long long n_iter, long long burn_in, bool sampling, long long every, double* seconds_out, Report report,
                     Step step) {
  auto t0 = std::chrono::steady_clock::now();
  for (long long i = 0; i < n_iter; ++i) {
    if (sampling && (i % every == 0 || i == burn_in)) {
      RC(report(i));
      if (i == burn_in) {
        RC(sync(ctx));
        t0 = std::chrono::steady_clock::now();
      }
    }
    step(i);
    HIPCK(hipGetLastError());
    flow_tick(ctx);
  }
  RC(sync(ctx));
  if (seconds_out) *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  return RMHMC_OK;
}

// device state of one IWLS call, taken from mem into p: l() of cur / trj ([2][n]), the saturated flag and count, m(cur.w)
int iwls_alloc(rmhmc_ctx* ctx, CallMem& mem, IwlsParams& p, int32_t compat) {
  const size_t n = ctx->n;
  RC(mem.alloc(&p.lq_cur, sizeof(double) * 2 * n));
  RC(mem.alloc(&p.sat, sizeof(int) * n));
  RC(mem.alloc(&p.nsat, sizeof(long long) * n));
  RC(mem.alloc(&p.mcur, sizeof(double) * n * ctx->DP));
  HIPCK(hipMemsetAsync(p.lq_cur, 0, sizeof(double) * 2 * n, ctx->stream));
  HIPCK(hipMemsetAsync(p.nsat, 0, sizeof(long long) * n, ctx->stream));
  p.compat = compat ? 1 : 0;
  p.lq_trj = p.lq_cur + n;
  return RMHMC_OK;
}

void launch_iwls_ljit(rmhmc_ctx* ctx, Group& g, const double* Ginv, double* out) {
  launch(ctx, "iwls", [&](hipStream_t st) {
    NB_SWITCH(ctx, hipLaunchKernelGGL((k_iwls_ljit<NB_>), dim3((unsigned)g.n), dim3(64), 0, st, ctx->D, ctx->DP, Ginv, out));
  });
}

// one iteration of every chain: proposal, the point evaluation at w' (mode 1, the assembly path of the context's flags), compat terms,
// decision
void launch_iwls_iter(rmhmc_ctx* ctx, Group& g, const IwlsParams& p) {
  SMALL(ctx, g, "iwls", k_iwls_begin, ctx->D, ctx->DP, g.ch, p);
  eval_point_phases(ctx, g, nullptr, 1);
  if (p.compat) {
    launch_iwls_ljit(ctx, g, g.ch.trj.Ginv, p.lq_trj);
    launch(ctx, "iwls_sat", [&](hipStream_t st) {
      const dim3 grid((unsigned)((ctx->M + IWLS_SAT_ROWS - 1) / IWLS_SAT_ROWS), (unsigned)((g.n + IWLS_SAT_CH - 1) / IWLS_SAT_CH));
      hipLaunchKernelGGL(k_iwls_sat, grid, dim3(IWLS_SAT_ROWS), 0, st, ctx->dd, g.n, (const double*)g.ch.trj.w, p.sat);
    });
  }
  SMALL(ctx, g, "iwls", k_iwls_end, ctx->D, ctx->DP, g.ch, p);
}

// Iterations 0..n_iter-1 of every chain (iwls.py:38-85) from the record at theta0 (default 0, :18), evaluated by the generic kernels
// (the arithmetic of the iterations' own evaluations).  Sampling: the reference's reports before iterations i % 1000 == 0 and burn_in
// (:39-43), then the timer.
int iwls_run(rmhmc_ctx* ctx, IwlsParams p, long long n_iter, bool sampling, const double* theta0, double* seconds_out) {
  Group& g = ctx->batch;
  RC(mmala_init(ctx, theta0, false));
  if (p.compat) launch_iwls_ljit(ctx, g, g.ch.cur.Ginv, p.lq_cur);
  std::vector<long long> acc;
  const auto report = [&](long long i) -> int {
    if (!ctx->progress_fn) return RMHMC_OK;
    acc.resize(ctx->n);
    RC(download(ctx, acc.data(), ctx->batch.ch.accepted, ctx->n));
    RC(sync(ctx));
    long long a = 0;
    for (long long x : acc) a += x;
    if (i % 1000 == 0) ctx->progress_fn(RMHMC_EV_PROGRESS, i, a, i * ctx->n, ctx->progress_user);
    if (i == p.burn_in) ctx->progress_fn(RMHMC_EV_BURNIN_DONE, i, a, i * ctx->n, ctx->progress_user);
    return RMHMC_OK;
  };
  return timed_iterations(ctx, n_iter, p.burn_in, sampling, 1000, seconds_out, report, [&](long long i) {
    p.it = i;
    launch_iwls_iter(ctx, g, p);
  });
}

int iwls_sample_body(rmhmc_ctx* ctx, const char* who, int64_t n_iter, int64_t burn_in, int32_t compat, uint64_t seed, int64_t chain_offset,
                     const double* theta0, const rmhmc_out& out, int64_t* accepted_out, int64_t* saturated_out, double* seconds_out) {
  if (!amh_iters_ok(n_iter, burn_in) || chain_offset < 0)
    return fail(ctx, RMHMC_ERR_INVALID, std::string(who) + ": need 0 <= burn_in < n_iter < 2^32, chain_offset >= 0");
  RC(stats_limit(ctx, who, out, n_iter - burn_in));
  if (ctx->D > 64) return fail(ctx, RMHMC_ERR_UNSUPPORTED, kIwlsDMsg);
  ctx->chains_ready = false;
  const int64_t S = n_iter - burn_in;
  CallMem mem(ctx);  // (outside the core: the copy of nsat that counter_out queues is drained by write_out)
  return sample_to(ctx, S, out, [&](double* d_samples) -> int {
    IwlsParams p{};
    RC(iwls_alloc(ctx, mem, p, compat));
    p.seed = seed; p.chain_offset = chain_offset; p.burn_in = burn_in; p.S = S; p.samples = d_samples; p.T = n_iter;
    RC(iwls_run(ctx, p, n_iter, true, theta0, seconds_out));
    RC(counter_out(ctx, out, accepted_out, ctx->batch.ch.accepted));
    return counter_out(ctx, out, saturated_out, p.nsat);
  });
}

}  // namespace

extern "C" {

int rmhmc_iwls_sample(rmhmc_ctx* ctx, int64_t n_iter, int64_t burn_in, int32_t compat, uint64_t seed, int64_t chain_offset,
                      const double* theta0, double* samples_out, int64_t* accepted_out, int64_t* saturated_out, double* seconds_out) {
  NEED_DATA(ctx);
  if (!samples_out) return fail(ctx, RMHMC_ERR_INVALID, "iwls_sample: need samples_out");
  return iwls_sample_body(ctx, "iwls_sample", n_iter, burn_in, compat, seed, chain_offset, theta0, {RMHMC_OUT_HOST, samples_out}, accepted_out,
                          saturated_out, seconds_out);
}
int rmhmc_iwls_sample_to(rmhmc_ctx* ctx, int64_t n_iter, int64_t burn_in, int32_t compat, uint64_t seed, int64_t chain_offset,
                         const double* theta0, const rmhmc_out* out, int64_t* accepted_out, int64_t* saturated_out, double* seconds_out) {
  NEED_DATA(ctx);
  RC(out_check(ctx, "iwls_sample_to", out));
  return iwls_sample_body(ctx, "iwls_sample_to", n_iter, burn_in, compat, seed, chain_offset, theta0, *out, accepted_out, saturated_out,
                          seconds_out);
}

int rmhmc_iwls_replay(rmhmc_ctx* ctx, int64_t n_iter, int32_t compat, const double* w_prop, const double* u, const double* theta0,
                      double* w_out, double* mean_out, double* ljl_out, double* ratio_out, int8_t* decisions_out) {
  NEED_DATA(ctx);
  if (!w_prop || !u || !w_out || n_iter < 1 || n_iter > (int64_t)0xffffffffLL)
    return fail(ctx, RMHMC_ERR_INVALID, "iwls_replay: need w_prop, u, w_out and 0 < n_iter < 2^32");
  if (ctx->D > 64) return fail(ctx, RMHMC_ERR_UNSUPPORTED, kIwlsDMsg);
  ctx->chains_ready = false;
  const size_t n = ctx->n, D = ctx->D, T = (size_t)n_iter, vec = n * T * D;
  CallMem mem(ctx);
  double *d_wp = nullptr, *d_u = nullptr, *d_w = nullptr, *d_m = nullptr, *d_l = nullptr, *d_r = nullptr;
  int8_t* d_dec = nullptr;
  RC(mem.alloc(&d_wp, sizeof(double) * vec)); RC(mem.alloc(&d_u, sizeof(double) * n * T));
  RC(mem.alloc(&d_w, sizeof(double) * vec)); RC(mem.alloc(&d_m, sizeof(double) * vec));
  RC(mem.alloc(&d_l, sizeof(double) * n * T)); RC(mem.alloc(&d_r, sizeof(double) * n * T));
  RC(mem.alloc(&d_dec, n * T));
  RC(upload(ctx, d_wp, w_prop, vec)); RC(upload(ctx, d_u, u, n * T));
  IwlsParams p{};
  RC(iwls_alloc(ctx, mem, p, compat));
  p.T = n_iter; p.w_prop = d_wp; p.u_in = d_u; p.w_out = d_w; p.mean_out = d_m; p.ljl_out = d_l; p.ratio_out = d_r; p.dec_out = d_dec;
  RC(iwls_run(ctx, p, n_iter, false, theta0, nullptr));
  RC(download(ctx, w_out, d_w, vec));
  if (mean_out) RC(download(ctx, mean_out, d_m, vec));
  if (ljl_out) RC(download(ctx, ljl_out, d_l, n * T));
  if (ratio_out) RC(download(ctx, ratio_out, d_r, n * T));
  if (decisions_out) RC(download(ctx, decisions_out, d_dec, n * T));
  return sync(ctx);
}

}  // extern "C"

// ---- auxiliary-variable Gibbs sampler (gibbs_sampler.py, gibbs.hip.h) --------------------------------------------------------------
namespace {

const char* const kGibbsDMsg = "gibbs: D > 64 is not supported (64 < D <= 256 needs a blocked inverse and sweep)";

// device state of one Gibbs call, taken from mem into p; G, V and Lt are the context's Gq, trj.Ginv and trj.L
int gibbs_alloc(rmhmc_ctx* ctx, CallMem& mem, GibbsParams& p) {
  const size_t n = ctx->n, Mp = ctx->Mp, DP = ctx->DP;
  RC(mem.alloc(&p.Z, sizeof(double) * n * Mp)); RC(mem.alloc(&p.lam, sizeof(double) * n * Mp));
  RC(mem.alloc(&p.ilam, sizeof(double) * n * Mp));
  RC(mem.alloc(&p.B, sizeof(double) * n * DP)); RC(mem.alloc(&p.beta, sizeof(double) * n * DP));
  RC(mem.alloc(&p.capped, sizeof(long long) * n)); RC(mem.alloc(&p.stop, sizeof(int) * n));
  RC(mem.alloc(&p.dead, sizeof(long long) * n));
  HIPCK(hipMemsetAsync(p.B, 0, sizeof(double) * n * DP, ctx->stream));
  HIPCK(hipMemsetAsync(p.beta, 0, sizeof(double) * n * DP, ctx->stream));
  p.G = ctx->batch.ch.Gq; p.V = ctx->batch.ch.trj.Ginv; p.Lt = ctx->batch.ch.trj.L;
  return RMHMC_OK;
}

// one iteration of every chain
void launch_gibbs_iter(rmhmc_ctx* ctx, const GibbsParams& p) {
  const unsigned n = (unsigned)ctx->n;
  const int D = (int)ctx->D, DP = (int)ctx->DP;
  launch(ctx, "gibbs_assemble", [&](hipStream_t st) {  // (one row range per chain whatever the batch: see gibbs.hip.h)
    NB_SWITCH(ctx, hipLaunchKernelGGL((k_assemble<NB_>), dim3((n + 3) / 4), dim3(256), 0, st, ctx->dd, (int)n, ctx->batch.ch.phase,
                                      (const double*)p.ilam, p.G, (size_t)0));
  });
  launch(ctx, "gibbs_factor", [&](hipStream_t st) {
    NB_SWITCH(ctx, hipLaunchKernelGGL((k_gibbs_factor<NB_>), dim3(n), dim3(64), 0, st, D, DP, p));
  });
  launch(ctx, "gibbs_b", [&](hipStream_t st) { hipLaunchKernelGGL(k_gibbs_b, dim3(n), dim3(256), 0, st, ctx->dd, p); });
  launch(ctx, "gibbs_sweep", [&](hipStream_t st) {
    NB_SWITCH(ctx, hipLaunchKernelGGL((k_gibbs_sweep<NB_>), dim3(n), dim3(64), 0, st, ctx->dd, p));
  });
  launch(ctx, "gibbs_beta", [&](hipStream_t st) { hipLaunchKernelGGL(k_gibbs_beta, dim3(n), dim3(64), 0, st, D, DP, p); });
  launch(ctx, "gibbs_mix", [&](hipStream_t st) {
    hipLaunchKernelGGL(k_gibbs_mix, dim3(n, (unsigned)((ctx->M + GIBBS_MIX_ROWS - 1) / GIBBS_MIX_ROWS)), dim3(GIBBS_MIX_ROWS), 0, st, ctx->dd, p);
  });
}

// Initialisation and iterations 0..n_iter-1 of every chain.  Sampling: the host synchronises only before the iterations the reference
// prints on (i % 100 == 0, gibbs_sampler.py:97-98) and before iteration burn_in, where the timer starts (:100-101).
int gibbs_run_body(rmhmc_ctx* ctx, GibbsParams p, long long n_iter, bool sampling, double* seconds_out) {
  fill_int(ctx, ctx->batch.ch.phase, 1, ctx->n);
  hipLaunchKernelGGL(k_gibbs_init, dim3((unsigned)ctx->n, (unsigned)((ctx->Mp + 255) / 256)), dim3(256), 0, ctx->stream, ctx->dd, p);
  HIPCK(hipGetLastError());
  const auto report = [&](long long i) -> int {
    if (i % 100 != 0 || !ctx->progress_fn) return RMHMC_OK;
    RC(sync(ctx));
    ctx->progress_fn(RMHMC_EV_PROGRESS, i, 0, i * ctx->n, ctx->progress_user);
    return RMHMC_OK;
  };
  return timed_iterations(ctx, n_iter, p.burn_in, sampling, 100, seconds_out, report, [&](long long i) {
    p.it = i;
    launch_gibbs_iter(ctx, p);
  });
}
int gibbs_run(rmhmc_ctx* ctx, const GibbsParams& p, long long n_iter, bool sampling, double* seconds_out) {
  const int rc = gibbs_run_body(ctx, p, n_iter, sampling, seconds_out);
  fill_int(ctx, ctx->batch.ch.phase, 0, ctx->n);  // on every path: the next user of the context finds the phases as gibbs_run found them
  return rc;
}

// Z_host, lam_host: [n][N] in host memory whatever the descriptor says, or NULL - the final state that rmhmc_gibbs_sample returns and
// rmhmc_gibbs_sample_to does not; copied while the state of the call is alive
int gibbs_sample_body(rmhmc_ctx* ctx, const char* who, int64_t n_iter, int64_t burn_in, uint64_t seed, int64_t chain_offset, const rmhmc_out& out,
                      int64_t* capped_out, int64_t* stopped_out, double* Z_host, double* lam_host, double* seconds_out) {
  if (!amh_iters_ok(n_iter, burn_in) || chain_offset < 0 || chain_offset + ctx->n > (int64_t)1 << 32)
    return fail(ctx, RMHMC_ERR_INVALID, std::string(who) + ": need 0 <= burn_in < n_iter < 2^32, 0 <= chain_offset, chain_offset + n <= 2^32");
  RC(stats_limit(ctx, who, out, n_iter - burn_in));
  if (ctx->D > 64) return fail(ctx, RMHMC_ERR_UNSUPPORTED, kGibbsDMsg);
  ctx->chains_ready = false;
  const int64_t S = n_iter - burn_in;
  CallMem mem(ctx);  // (outside the core: the copies that it queues from the state of the call are drained by write_out)
  return sample_to(ctx, S, out, [&](double* d_samples) -> int {
    HIPCK(hipMemsetAsync(d_samples, 0xff, sizeof(double) * (size_t)ctx->n * (size_t)S * ctx->D, ctx->stream));  // NaN: the rows a stopped chain never writes
    GibbsParams p{};
    RC(gibbs_alloc(ctx, mem, p));
    p.seed = seed; p.chain_offset = chain_offset; p.burn_in = burn_in; p.S = S; p.samples = d_samples; p.T = n_iter;
    RC(gibbs_run(ctx, p, n_iter, true, seconds_out));
    const size_t n = ctx->n, N = ctx->M, Mp = ctx->Mp;  // [n][Mp] -> [n][N]
    if (Z_host) RC(copy_rows(ctx, Z_host, N, p.Z, Mp, N, n, hipMemcpyDeviceToHost));
    if (lam_host) RC(copy_rows(ctx, lam_host, N, p.lam, Mp, N, n, hipMemcpyDeviceToHost));
    RC(counter_out(ctx, out, capped_out, p.capped));
    return counter_out(ctx, out, stopped_out, p.dead);
  });
}

}  // namespace

extern "C" {

int rmhmc_gibbs_sample(rmhmc_ctx* ctx, int64_t n_iter, int64_t burn_in, uint64_t seed, int64_t chain_offset, double* samples_out,
                       int64_t* capped_out, int64_t* stopped_out, double* Z_out, double* lam_out, double* seconds_out) {
  NEED_DATA(ctx);
  if (!samples_out) return fail(ctx, RMHMC_ERR_INVALID, "gibbs_sample: need samples_out");
  return gibbs_sample_body(ctx, "gibbs_sample", n_iter, burn_in, seed, chain_offset, {RMHMC_OUT_HOST, samples_out}, capped_out, stopped_out,
                           Z_out, lam_out, seconds_out);
}
int rmhmc_gibbs_sample_to(rmhmc_ctx* ctx, int64_t n_iter, int64_t burn_in, uint64_t seed, int64_t chain_offset, const rmhmc_out* out,
                          int64_t* capped_out, int64_t* stopped_out, double* seconds_out) {
  NEED_DATA(ctx);
  RC(out_check(ctx, "gibbs_sample_to", out));
  return gibbs_sample_body(ctx, "gibbs_sample_to", n_iter, burn_in, seed, chain_offset, *out, capped_out, stopped_out, nullptr, nullptr,
                           seconds_out);
}

int rmhmc_gibbs_replay(rmhmc_ctx* ctx, int64_t n_iter, const double* u_init, const double* u_sweep, const double* T, const double* ks_draws,
                       const int64_t* ks_offset, int64_t ks_total, double* beta_out, double* B_out, int32_t* attempts_out, double* Z_out,
                       double* lam_out, int64_t* capped_out, int32_t* status_out) {
  NEED_DATA(ctx);
  if (!u_init || !u_sweep || !T || !ks_draws || !ks_offset || !beta_out || !B_out || !attempts_out || ks_total < 0 || n_iter < 1 ||
      n_iter > (int64_t)0xffffffffLL)
    return fail(ctx, RMHMC_ERR_INVALID, "gibbs_replay: need the five tapes, beta_out, B_out, attempts_out, ks_total >= 0 and 0 < n_iter < 2^32");
  if (ctx->D > 64) return fail(ctx, RMHMC_ERR_UNSUPPORTED, kGibbsDMsg);
  const size_t n = ctx->n, D = ctx->D, N = ctx->M, Tn = (size_t)n_iter, Mp = ctx->Mp;
  for (size_t r = 0; r < n * Tn; ++r)  // every row's range lies inside its chain's draws
    for (size_t j = 0; j <= N; ++j) {
      const int64_t o = ks_offset[r * (N + 1) + j];
      if (o < 0 || o > ks_total || (j && o < ks_offset[r * (N + 1) + j - 1]))
        return fail(ctx, RMHMC_ERR_INVALID, "gibbs_replay: ks_offset must be non-decreasing within 0..ks_total");
    }
  HIPCK(hipSetDevice(ctx->device));
  ctx->chains_ready = false;
  CallMem mem(ctx);
  double *d_ui = nullptr, *d_us = nullptr, *d_T = nullptr, *d_ks = nullptr, *d_beta = nullptr, *d_B = nullptr;
  long long* d_off = nullptr;
  int* d_att = nullptr;
  const size_t nks = n * (size_t)std::max<int64_t>(ks_total, 1) * 3;
  RC(mem.alloc(&d_ui, sizeof(double) * n * N)); RC(mem.alloc(&d_us, sizeof(double) * n * Tn * N));
  RC(mem.alloc(&d_T, sizeof(double) * n * Tn * D)); RC(mem.alloc(&d_ks, sizeof(double) * nks));
  RC(mem.alloc(&d_off, sizeof(long long) * n * Tn * (N + 1)));
  RC(mem.alloc(&d_beta, sizeof(double) * n * Tn * D)); RC(mem.alloc(&d_B, sizeof(double) * n * Tn * D));
  RC(mem.alloc(&d_att, sizeof(int) * n * Tn * N));
  HIPCK(hipMemsetAsync(d_beta, 0, sizeof(double) * n * Tn * D, ctx->stream)); HIPCK(hipMemsetAsync(d_B, 0, sizeof(double) * n * Tn * D, ctx->stream));
  HIPCK(hipMemsetAsync(d_att, 0, sizeof(int) * n * Tn * N, ctx->stream));
  RC(upload(ctx, d_ui, u_init, n * N)); RC(upload(ctx, d_us, u_sweep, n * Tn * N)); RC(upload(ctx, d_T, T, n * Tn * D));
  if (ks_total) RC(upload(ctx, d_ks, ks_draws, n * (size_t)ks_total * 3));
  static_assert(sizeof(long long) == sizeof(int64_t), "int64");
  RC(upload(ctx, d_off, (const long long*)ks_offset, n * Tn * (N + 1)));
  GibbsParams p{};
  RC(gibbs_alloc(ctx, mem, p));
  p.T = n_iter; p.u_init = d_ui; p.u_sweep = d_us; p.T_in = d_T; p.ks = d_ks; p.ks_off = d_off; p.ks_total = ks_total;
  p.beta_out = d_beta; p.B_out = d_B; p.att_out = d_att; p.burn_in = n_iter;
  RC(gibbs_run(ctx, p, n_iter, false, nullptr));
  RC(download(ctx, beta_out, d_beta, n * Tn * D)); RC(download(ctx, B_out, d_B, n * Tn * D));
  RC(download(ctx, (int*)attempts_out, d_att, n * Tn * N));
  if (Z_out) RC(copy_rows(ctx, Z_out, N, p.Z, Mp, N, n, hipMemcpyDeviceToHost));
  if (lam_out) RC(copy_rows(ctx, lam_out, N, p.lam, Mp, N, n, hipMemcpyDeviceToHost));
  std::vector<long long> cp(n);
  std::vector<int> sp(n);
  RC(download(ctx, cp.data(), p.capped, n)); RC(download(ctx, sp.data(), p.stop, n));
  RC(sync(ctx));
  for (size_t c = 0; c < n; ++c) {
    if (capped_out) capped_out[c] = cp[c];
    if (status_out) status_out[c] = sp[c];
  }
  return RMHMC_OK;
}

}  // extern "C"

// ---- cross-chain diagnostics: split R-hat and the pooled ESS (include/rmhmc_diag.h, diag.h, diag.hip.h) ----------------------------
namespace {

template <int TW, int NQ>
int launch_diag_acov(rmhmc_ctx* ctx, dim3 grid, size_t lds, const double* d_samples, long long n, long long S, int P, int H, int T, int rows,
                     double* d_blk, double* d_means) {
  RC(raise_lds(ctx, (k_diag_acov<TW, NQ>), MAX_LDS));  // per device: set where it is used
  hipLaunchKernelGGL((k_diag_acov<TW, NQ>), grid, dim3(DIAG_THREADS), lds, ctx->stream, d_samples, n, S, P, H, T, rows, d_blk, d_means);
  return RMHMC_OK;
}

// samples [n][S][P] -> the partial [(4 + T)][P], all in device memory; queued on the stream, its two scratch buffers taken from mem,
// which the caller keeps until the stream is idle
int launch_diag(rmhmc_ctx* ctx, const double* d_samples, long long n, long long S, int P, long long T, double* d_partial, CallMem& mem) {
  const long long H = S / 2;
  const int tw = diag_tile_width(H, P);
  const long long nblocks = (n + DIAG_CHAINS - 1) / DIAG_CHAINS;
  if (tw < 1) return fail(ctx, RMHMC_ERR_UNSUPPORTED, "diag: the half series does not fit the LDS");
  const int nq = diag_lag_sets(T, tw);
  const long long ntiles = ((long long)P + tw - 1) / tw;
  if (T > nq * diag_lags_per_block(tw)) return fail(ctx, RMHMC_ERR_UNSUPPORTED, "diag: more lags than a workgroup holds");  // (never: diag.h)
  if (nblocks > 65535 || ntiles > 0x7fffffffLL) return fail(ctx, RMHMC_ERR_UNSUPPORTED, "diag: at most 65535 * 32 chains per call");
  const size_t rowlen = (size_t)(2 + T) * P;
  double *d_blk = nullptr, *d_means = nullptr;
  RC(mem.alloc(&d_blk, sizeof(double) * (size_t)nblocks * rowlen));
  RC(mem.alloc(&d_means, sizeof(double) * 2 * (size_t)n * P));
  const dim3 grid((unsigned)ntiles, (unsigned)nblocks);
  const size_t lds = (size_t)diag_lds_bytes(H, tw);
  const int rows = (int)diag_lds_rows(H);
  TW_SWITCH(tw, return fail(ctx, RMHMC_ERR_RUNTIME, "diag: no kernel for this tile width"),
            if (nq == 1) RC((launch_diag_acov<TW_, 1>(ctx, grid, lds, d_samples, n, S, P, (int)H, (int)T, rows, d_blk, d_means)));
            else RC((launch_diag_acov<TW_, DIAG_NQ>(ctx, grid, lds, d_samples, n, S, P, (int)H, (int)T, rows, d_blk, d_means))));
  hipLaunchKernelGGL(k_diag_reduce, dim3((unsigned)((rowlen + 255) / 256)), dim3(256), 0, ctx->stream, d_blk, nblocks, P, (int)H, (int)T, d_partial);
  hipLaunchKernelGGL(k_diag_m2, dim3((unsigned)((P + 15) / 16)), dim3(1024), 0, ctx->stream, d_means, 2 * n, P, d_partial);
  HIPCK(hipGetLastError());
  return RMHMC_OK;
}

}  // namespace

extern "C" {

int rmhmc_diag_partial_dev(rmhmc_ctx* ctx, const double* samples_dev, int64_t n, int64_t S, int32_t P, int64_t max_lag, double* partial_dev) {
  if (!ctx || !samples_dev || !partial_dev || n < 1 || P < 1 || max_lag < 0) return fail(ctx, RMHMC_ERR_INVALID, "diag_partial_dev: bad argument");
  if (S < 4 || S > 20000) return fail(ctx, RMHMC_ERR_UNSUPPORTED, "diag: 4 <= S <= 20000 samples per chain (the centred series is held in LDS)");
  const int64_t H = S / 2;
  if (max_lag > H - 1) return fail(ctx, RMHMC_ERR_INVALID, "diag_partial_dev: max_lag must be 0 (every lag) or 1 .. S/2 - 1");
  const int64_t T = (max_lag ? max_lag : H - 1) + 1;
  HIPCK(hipSetDevice(ctx->device));
  CallMem mem(ctx);
  return sync_after(ctx, launch_diag(ctx, samples_dev, n, S, P, T, partial_dev, mem));
}

int rmhmc_diag_finish(const double* const* partials, int32_t k, int64_t H, int64_t T, int32_t P, double* merged, double* rhat, double* ess,
                      int64_t* pairs, int64_t* chains_used) {
  const int rc = diag_finish(partials, k, H, T, P, merged, rhat, ess, pairs, chains_used);
  return rc == RMHMC_OK ? rc : fail(nullptr, rc, rc == RMHMC_ERR_NOMEM ? "diag_finish: out of memory"
                                                                       : "diag_finish: need k >= 1, H >= 2, 2 <= T <= H, P >= 1 and no NULL partial");
}

}  // extern "C"

// ---- posterior quantiles: the radix select on integer histograms (include/rmhmc_quant.h, quant.h, quant.hip.h) -----------------------
namespace {

template <int TW>
int launch_quant_tw(rmhmc_ctx* ctx, dim3 grid, const double* d_samples, long long N, int P, int round, int Kh, const unsigned long long* d_prefix,
                    const signed char* d_rep, unsigned long long* d_cnt) {
  RC(raise_lds(ctx, k_quant_hist<TW>, MAX_LDS));  // per device: set where it is used
  hipLaunchKernelGGL(k_quant_hist<TW>, grid, dim3(QUANT_THREADS), QUANT_LDS_BYTES, ctx->stream, d_samples, N, P, round, Kh, d_prefix, d_rep, d_cnt);
  return RMHMC_OK;
}

// samples [N][P] -> the histogram partial [Kh][P][256] of `round`, all in device memory; queued on the stream, its buffers taken from mem,
// which the caller keeps until the stream is idle.  prefix: host [K][P], unused in round 0
// (pre: buffers of the caller's for the counters [Kh][P][256], the prefixes and the representatives [K][P] in place of mem's)
struct QuantScratch { unsigned long long* cnt; unsigned long long* prefix; signed char* rep; };
int launch_quant_hist(rmhmc_ctx* ctx, const double* d_samples, long long N, int P, int round, const uint64_t* prefix, int K, double* d_hist,
                      CallMem& mem, const QuantScratch* pre = nullptr) {
  const int tw = quant_tile_width(P), Kh = round ? K : 1;
  const long long nblocks = (N + quant_block_rows(tw) - 1) / quant_block_rows(tw), ntiles = ((long long)P + tw - 1) / tw;
  if (nblocks > 0x7fffffffLL || ntiles > 65535) return fail(ctx, RMHMC_ERR_UNSUPPORTED, "quant: too many rows or columns for one launch");
  const size_t targets = (size_t)Kh * P, total = targets * QUANT_BINS;
  unsigned long long *d_cnt = nullptr, *d_prefix = nullptr;
  signed char* d_rep = nullptr;
  if (pre) d_cnt = pre->cnt;
  else RC(mem.alloc(&d_cnt, sizeof(unsigned long long) * total));
  HIPCK(hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long) * total, ctx->stream));
  if (round) {
    // a target whose top 8 round bits repeat those of an earlier target of its column is not counted again (k_quant_out copies)
    std::vector<signed char> rep(targets);
    for (int k = 0; k < K; ++k)
      for (int d = 0; d < P; ++d) {
        int first = 0;
        while (!quant_match(prefix[(size_t)first * P + d], prefix[(size_t)k * P + d], round)) ++first;
        rep[(size_t)k * P + d] = (signed char)first;
      }
    if (pre) { d_prefix = pre->prefix; d_rep = pre->rep; }
    else {
      RC(mem.alloc(&d_prefix, sizeof(uint64_t) * targets));
      RC(mem.alloc(&d_rep, targets));
    }
    HIPCK(hipMemcpyAsync(d_prefix, prefix, sizeof(uint64_t) * targets, hipMemcpyHostToDevice, ctx->stream));
    HIPCK(hipMemcpyAsync(d_rep, rep.data(), targets, hipMemcpyHostToDevice, ctx->stream));
    HIPCK(hipStreamSynchronize(ctx->stream));  // rep goes out of scope, and the caller's prefix is its own again
  }
  const dim3 grid((unsigned)nblocks, (unsigned)ntiles);
  int rc = RMHMC_OK;
  launch(ctx, "quant_hist", [&](hipStream_t) {
    TW_SWITCH(tw, rc = fail(ctx, RMHMC_ERR_RUNTIME, "quant: no kernel for this tile width"),
              rc = launch_quant_tw<TW_>(ctx, grid, d_samples, N, P, round, Kh, d_prefix, d_rep, d_cnt));
  });
  RC(rc);
  hipLaunchKernelGGL(k_quant_out, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, d_cnt, d_rep, P, total, d_hist);
  HIPCK(hipGetLastError());
  return RMHMC_OK;
}

const char* quant_hist_refusal(const rmhmc_ctx* ctx, const void* samples, int64_t n, int64_t S, int32_t P) {
  if (!ctx || !samples || n < 1 || S < 1 || P < 1 || n > INT64_MAX / S) return "need a context, samples, n >= 1, S >= 1, P >= 1";
  return nullptr;
}

}  // namespace

extern "C" {

int rmhmc_quant_hist_dev(rmhmc_ctx* ctx, const double* samples_dev, int64_t n, int64_t S, int32_t P, int32_t round, const uint64_t* prefix,
                         int32_t K, double* hist_dev) {
  if (const char* why = quant_hist_refusal(ctx, samples_dev, n, S, P)) return fail(ctx, RMHMC_ERR_INVALID, std::string("quant_hist_dev: ") + why);
  if (!hist_dev || round < 0 || round > 7 || K < 1 || K > QUANT_MAX_K || (round && !prefix))
    return fail(ctx, RMHMC_ERR_INVALID, "quant_hist_dev: need a histogram, 0 <= round <= 7, 1 <= K <= 16 and a prefix after round 0");
  if ((int64_t)K * P > INT32_MAX / QUANT_BINS) return fail(ctx, RMHMC_ERR_UNSUPPORTED, "quant_hist_dev: K * P * 256 must fit 31 bits");
  HIPCK(hipSetDevice(ctx->device));
  CallMem mem(ctx);
  return sync_after(ctx, launch_quant_hist(ctx, samples_dev, n * S, P, round, prefix, K, hist_dev, mem));
}

int rmhmc_quant_plan(const int64_t* m, const double* probs, int32_t Q, int32_t P, int64_t* rank, double* frac) {
  const int rc = quant_plan(m, probs, Q, P, rank, frac);
  return rc == RMHMC_OK ? rc : fail(nullptr, rc, "quant_plan: need m >= 0, 1 <= Q <= 8 probabilities in [0, 1], P >= 1 and no NULL pointer");
}

int rmhmc_quant_step(const double* const* hists, int32_t k_parts, int32_t P, int32_t K, int32_t round, uint64_t* prefix, int64_t* rank) {
  const int rc = quant_step(hists, k_parts, P, K, round, prefix, rank);
  return rc == RMHMC_OK ? rc : fail(nullptr, rc, rc == RMHMC_ERR_NOMEM ? "quant_step: out of memory"
                                                                       : "quant_step: bad argument, or a histogram that is not the one of this round of these targets");
}

int rmhmc_quant_finish(const uint64_t* prefix, const double* frac, const int64_t* m, int32_t Q, int32_t P, double* quant) {
  const int rc = quant_finish(prefix, frac, m, Q, P, quant);
  return rc == RMHMC_OK ? rc : fail(nullptr, rc, "quant_finish: need 1 <= Q <= 8, P >= 1 and no NULL pointer");
}

int rmhmc_quant_dev(rmhmc_ctx* ctx, const double* samples_dev, int64_t n, int64_t S, int32_t P, const double* probs, int32_t Q, double* quant,
                    int64_t* draws_used) {
  if (const char* why = quant_hist_refusal(ctx, samples_dev, n, S, P)) return fail(ctx, RMHMC_ERR_INVALID, std::string("quant_dev: ") + why);
  if (!probs || !quant || Q < 1 || Q > QUANT_MAX_Q) return fail(ctx, RMHMC_ERR_INVALID, "quant_dev: need 1 <= Q <= 8 probabilities and an output");
  for (int32_t j = 0; j < Q; ++j)
    if (!(probs[j] >= 0.0 && probs[j] <= 1.0)) return fail(ctx, RMHMC_ERR_INVALID, "quant_dev: a probability is outside [0, 1]");
  const int K = 2 * Q;
  if ((int64_t)K * P > INT32_MAX / QUANT_BINS) return fail(ctx, RMHMC_ERR_UNSUPPORTED, "quant_dev: 2 Q * P * 256 must fit 31 bits");
  HIPCK(hipSetDevice(ctx->device));
  const size_t targets = (size_t)K * P;
  std::vector<double> hist(targets * QUANT_BINS), frac((size_t)Q * P);
  std::vector<uint64_t> prefix(targets, 0);
  std::vector<int64_t> rank(targets), m((size_t)P);
  CallMem mem(ctx);
  double* d_hist = nullptr;
  RC(mem.alloc(&d_hist, sizeof(double) * hist.size()));
  for (int round = 0; round < 8; ++round) {
    const size_t len = (round ? targets : (size_t)P) * QUANT_BINS;
    int rc;
    {
      CallMem round_mem(ctx);
      rc = launch_quant_hist(ctx, samples_dev, n * S, P, round, prefix.data(), K, d_hist, round_mem);
      if (rc == RMHMC_OK) {
        hipError_t e = hipMemcpyAsync(hist.data(), d_hist, sizeof(double) * len, hipMemcpyDeviceToHost, ctx->stream);
        if (e != hipSuccess) rc = fail(ctx, RMHMC_ERR_RUNTIME, std::string(hipGetErrorString(e)) + " in quant_dev");
      }
      rc = sync_after(ctx, rc);
    }
    RC(rc);
    if (round == 0) {
      quant_totals(hist.data(), P, m.data());
      RC(rmhmc_quant_plan(m.data(), probs, Q, P, rank.data(), frac.data()));
    }
    const double* one = hist.data();
    const int rs = quant_step(&one, 1, P, K, round, prefix.data(), rank.data());
    if (rs != RMHMC_OK) return fail(ctx, rs, "quant_dev: a round's histogram does not continue the previous round");
  }
  RC(rmhmc_quant_finish(prefix.data(), frac.data(), m.data(), Q, P, quant));
  if (draws_used)
    for (int32_t d = 0; d < P; ++d) draws_used[d] = m[(size_t)d];
  return RMHMC_OK;
}

}  // extern "C"

// ---- warm-up of the fixed-metric HMC sampler: pooled covariance, regularised mass, dual averaging (include/rmhmc_adapt.h, adapt.h,
// adapt.hip.h) ------------------------------------------------------------------------------------------------------------------------
namespace {

// samples [N][P] -> the partial [(2 + P)][P], all in device memory; queued on the stream, its scratch buffer taken from mem, which the
// caller keeps until the stream is idle
int launch_cov(rmhmc_ctx* ctx, const double* d_x, size_t N, int P, double* d_partial, CallMem& mem) {
  int64_t nb1, rpb1, nb2, rpb2;
  cov_plan_sums((int64_t)N, &nb1, &rpb1);
  cov_plan((int64_t)N, P, &nb2, &rpb2);
  const size_t p = (size_t)P, nt = (p + 15) / 16;
  const size_t doubles = (size_t)nb1 * 3 * p + 2 * p + (size_t)nb2 * p * p;
  double* blk = nullptr;
  RC(mem.alloc(&blk, sizeof(double) * doubles + N));
  double* ctr = blk + (size_t)nb1 * 3 * p;
  double* scr = ctr + 2 * p;
  unsigned char* valid = (unsigned char*)(scr + (size_t)nb2 * p * p);
  launch(ctx, "cov", [&](hipStream_t st) {
    hipLaunchKernelGGL(k_cov_sums, dim3((unsigned)nb1), dim3(256), 0, st, d_x, N, P, (size_t)rpb1, valid, blk);
    hipLaunchKernelGGL(k_cov_mean, dim3(1), dim3(256), 0, st, blk, (size_t)nb1, P, d_partial, ctr);
    hipLaunchKernelGGL(k_cov_xtx, dim3((unsigned)(nt * (nt + 1) / 2), (unsigned)nb2), dim3(64), 0, st, d_x, N, P, (size_t)rpb2, valid, ctr, scr);
    hipLaunchKernelGGL(k_cov_reduce, dim3((unsigned)((p * p + 255) / 256)), dim3(256), 0, st, scr, (size_t)nb2, P, d_partial);
  });
  HIPCK(hipGetLastError());
  return RMHMC_OK;
}

int cov_partial(rmhmc_ctx* ctx, const double* d_x, size_t N, int P, double* d_partial) {
  CallMem mem(ctx);
  return sync_after(ctx, launch_cov(ctx, d_x, N, P, d_partial, mem));
}

}  // namespace

extern "C" {

int rmhmc_cov_partial_dev(rmhmc_ctx* ctx, const double* samples_dev, int64_t n, int64_t S, int32_t P, double* partial_dev) {
  if (!ctx || !samples_dev || !partial_dev || n < 1 || S < 1 || P < 1 || n > INT64_MAX / S)
    return fail(ctx, RMHMC_ERR_INVALID, "cov_partial_dev: need samples, a partial, n >= 1, S >= 1, P >= 1");
  if (P > COV_MAX_P) return fail(ctx, RMHMC_ERR_UNSUPPORTED, "cov_partial_dev: P <= 256");
  HIPCK(hipSetDevice(ctx->device));
  return cov_partial(ctx, samples_dev, (size_t)n * (size_t)S, P, partial_dev);
}

int rmhmc_cov_finish(const double* const* partials, int32_t k, int32_t P, double* merged, double* mean, double* cov, int64_t* rows_used) {
  const int rc = cov_finish(partials, k, P, merged, mean, cov, rows_used);
  return rc == RMHMC_OK ? rc : fail(nullptr, rc, rc == RMHMC_ERR_NOMEM ? "cov_finish: out of memory" : "cov_finish: need k >= 1, P >= 1 and no NULL partial");
}

int rmhmc_adapt_mass(const double* cov, int64_t m, int32_t P, double* mass_out) {
  const char* why = "";
  const int rc = adapt_mass(cov, m, P, mass_out, &why);
  return rc == RMHMC_OK ? rc : fail(nullptr, rc, why);
}

int rmhmc_adapt_init(double state[4], double eps, double factor) {
  const int rc = adapt_init(state, eps, factor);
  return rc == RMHMC_OK ? rc : fail(nullptr, rc, "adapt_init: need a state, a finite step size > 0 and a finite factor > 0");
}

int rmhmc_adapt_step(double state[4], double accept, double delta, double gamma, double t0, double kappa, double* eps_next, double* eps_bar) {
  const int rc = adapt_step(state, accept, delta, gamma, t0, kappa, eps_next, eps_bar);
  return rc == RMHMC_OK ? rc : fail(nullptr, rc, "adapt_step: need a state, a finite acceptance statistic and a step size that stays finite and > 0");
}

int rmhmc_phmc_warmup(rmhmc_ctx* ctx, const double* theta0, int32_t L, double eps0, double delta, double gamma, double t0, double kappa,
                      uint64_t seed, int64_t chain_offset, int32_t W, const int64_t* win_len, const int32_t* win_kind, int64_t min_rows,
                      double* eps_out, double* mass_out, double* theta_out, double* eps_trace, double* accept_trace, int32_t* mass_updated,
                      double* seconds_out) {
  NEED_DATA(ctx);
  const auto t_start = std::chrono::steady_clock::now();
  if (!win_len || !win_kind || W < 1 || L < 1 || min_rows < 1 || !std::isfinite(eps0) || !(eps0 > 0.0))
    return fail(ctx, RMHMC_ERR_INVALID, "phmc_warmup: need a schedule of W >= 1 windows, L >= 1, min_rows >= 1 and a finite eps0 > 0");
  int64_t Kmax = 0;
  for (int32_t w = 0; w < W; ++w) {
    if (win_len[w] < 1 || (win_kind[w] != 0 && win_kind[w] != 1))
      return fail(ctx, RMHMC_ERR_INVALID, "phmc_warmup: every window needs a length >= 1 and a kind 0 or 1");
    Kmax = std::max<int64_t>(Kmax, win_len[w]);
  }
  if (!ctx->have_mass) return fail(ctx, RMHMC_ERR_INVALID, "phmc_warmup: rmhmc_phmc_set_mass has not been called");
  if (ctx->D > COV_MAX_P) return fail(ctx, RMHMC_ERR_UNSUPPORTED, "phmc_warmup: D <= 256");
  const size_t n = ctx->n, D = ctx->D, plen = (2 + D) * D;
  double state[4];
  RC(adapt_init(state, eps0, ADAPT_FACTOR_START) == RMHMC_OK ? RMHMC_OK : fail(ctx, RMHMC_ERR_INVALID, "phmc_warmup: bad eps0"));
  std::vector<double> theta, running(plen, 0.0), wpart(plen), merged(plen), cov(D * D), mass(D * D), mass_last(D * D, NAN);
  std::vector<long long> acc(n);
  if (theta0) theta.assign(theta0, theta0 + n * D);
  double eps = eps0, eps_bar = eps0;
  CallMem mem(ctx);
  double *d_win = nullptr, *d_part = nullptr;  // the samples of one window [n][K][D]; its partial
  RC(mem.alloc(&d_win, sizeof(double) * n * (size_t)Kmax * D));
  RC(mem.alloc(&d_part, sizeof(double) * plen));
  for (int32_t w = 0; w < W; ++w) {
    const int64_t K = win_len[w];
    ctx->chains_ready = false;
    const Run run{PHMC, L, 0, eps, seed + 1 + (uint64_t)w, chain_offset, nullptr};
    RC(hmc_sample_core(ctx, run, K, 0, theta.empty() ? nullptr : theta.data(), d_win, nullptr));
    RC(download(ctx, acc.data(), ctx->batch.ch.accepted, n));
    theta.resize(n * D);
    HIPCK(hipMemcpy2DAsync(theta.data(), D * sizeof(double), d_win + (size_t)(K - 1) * D, (size_t)K * D * sizeof(double), D * sizeof(double), n,
                           hipMemcpyDeviceToHost, ctx->stream));
    RC(sync(ctx));
    const double a = adapt_accept((const int64_t*)acc.data(), (int64_t)n, K);
    if (eps_trace) eps_trace[w] = eps;
    if (accept_trace) accept_trace[w] = a;
    if (mass_updated) mass_updated[w] = 0;
    double eps_next = eps;
    if (adapt_step(state, a, delta, gamma, t0, kappa, &eps_next, &eps_bar) != RMHMC_OK)
      return fail(ctx, RMHMC_ERR_INVALID, "phmc_warmup: the step size has left the finite positive numbers (dual averaging constants?)");
    eps = eps_next;
    if (win_kind[w] != 1) continue;
    RC(cov_partial(ctx, d_win, n * (size_t)K, (int)D, d_part));
    RC(download(ctx, wpart.data(), d_part, plen));
    RC(sync(ctx));
    const double* const two[2] = {running.data(), wpart.data()};
    int64_t m = 0;
    RC(cov_finish(two, 2, (int32_t)D, merged.data(), nullptr, cov.data(), &m));
    running = merged;
    if (m < min_rows) continue;
    const char* why = "";
    if (adapt_mass(cov.data(), m, (int32_t)D, mass.data(), &why) == RMHMC_OK && rmhmc_phmc_set_mass(ctx, mass.data()) == RMHMC_OK) {
      mass_last = mass;
      std::fill(running.begin(), running.end(), 0.0);
      (void)adapt_init(state, eps, ADAPT_FACTOR_RESTART);
      if (mass_updated) mass_updated[w] = 1;
    } else {  // refused: the previous mass stays
      if (mass_updated) mass_updated[w] = -1;
    }
  }
  if (eps_out) *eps_out = eps_bar;
  if (mass_out) std::copy(mass_last.begin(), mass_last.end(), mass_out);
  if (theta_out) std::copy(theta.begin(), theta.end(), theta_out);
  if (seconds_out) *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
  return RMHMC_OK;
}

}  // extern "C"

// ---- annealed importance sampling with tempered fixed-metric HMC (include/rmhmc_ais.h, ais.h, ais.hip.h) ----------------------------------
namespace {

// logw [n] -> the partial [5], all in device memory; synchronises
int ais_partial(rmhmc_ctx* ctx, const double* d_lw, size_t n, double* d_partial) {
  int64_t nb, pb;
  ais_plan((int64_t)n, &nb, &pb);
  CallMem mem(ctx);
  double* d_scr = nullptr;  // blk [nb][3], sums [nb][4]
  RC(mem.alloc(&d_scr, sizeof(double) * 7 * (size_t)nb));
  launch(ctx, "ais", [&](hipStream_t st) {
    hipLaunchKernelGGL(k_ais_max, dim3((unsigned)nb), dim3(256), 0, st, d_lw, n, (size_t)pb, d_scr);
    hipLaunchKernelGGL(k_ais_sums, dim3((unsigned)nb), dim3(256), 0, st, d_lw, n, (size_t)pb, (const double*)d_scr, (int)nb, d_scr + 3 * (size_t)nb);
    hipLaunchKernelGGL(k_ais_fin, dim3(1), dim3(64), 0, st, (const double*)d_scr, (const double*)(d_scr + 3 * (size_t)nb), (int)nb, d_partial);
  });
  const hipError_t e = hipGetLastError();
  const int rs = sync(ctx);
  if (e != hipSuccess) return fail(ctx, RMHMC_ERR_RUNTIME, std::string(hipGetErrorString(e)) + " in ais_partial");
  return rs;
}

// prior draws of key (seed, chain_offset + c) into out [n][ld] (device memory), queued on the stream
void launch_ais_prior(rmhmc_ctx* ctx, uint64_t seed, int64_t chain_offset, double* out, int ld) {
  launch(ctx, "ais", [&](hipStream_t st) {
    hipLaunchKernelGGL(k_ais_prior, dim3((unsigned)ctx->n), dim3(64), 0, st, ctx->D, (unsigned long long)seed, (long long)chain_offset,
                       std::sqrt(ctx->alpha), out, ld);
  });
}

int tphmc_sample_body(rmhmc_ctx* ctx, const char* who, int64_t n_iter, int64_t burn_in, int32_t L, double eps, uint64_t seed, int64_t chain_offset,
                      const double* theta0, const rmhmc_out& out, int64_t* accept_out, int64_t* steps_out, double* seconds_out, double beta,
                      double* loglik0_out, double* loglik_out) {
  if (burn_in < 0 || burn_in >= n_iter || L < 1) return fail(ctx, RMHMC_ERR_INVALID, std::string(who) + ": need 0 <= burn_in < n_iter, L >= 1");
  if (!ais_beta_ok(beta)) return fail(ctx, RMHMC_ERR_INVALID, std::string(who) + ": beta must be finite and >= 0");
  if (!ctx->have_mass) return fail(ctx, RMHMC_ERR_INVALID, std::string(who) + ": rmhmc_phmc_set_mass has not been called");
  RC(stats_limit(ctx, who, out, n_iter - burn_in));
  ctx->chains_ready = false;
  RC(ais_buffers(ctx));
  Run run{TPHMC, L, 0, eps, seed, chain_offset, nullptr};  // (no fixed-point iterations: no K)
  run.beta = beta;
  return sample_to(ctx, n_iter - burn_in, out, [&](double* d_samples) -> int {
    RC(tphmc_init_chains(ctx, theta0, beta));
    RC(hmc_sample_run(ctx, run, n_iter, burn_in, d_samples, seconds_out));
    RC(counter_out(ctx, out, accept_out, ctx->batch.ch.accepted));
    RC(counter_out(ctx, out, steps_out, ctx->d_steps0));
    if (loglik0_out) RC(download(ctx, loglik0_out, ctx->d_ais_ll0, ctx->n));
    if (loglik_out) RC(download(ctx, loglik_out, ctx->d_ais_ll, ctx->n));
    return RMHMC_OK;
  });
}

// ---- what the two annealing runs share (rmhmc_ais_run; rmhmc_smc_run below): their opening, a stage's mass and its tail, the weight summary.
// Their stage heads differ (a given ladder; a search, reweighting and resampling) and stay with them.
struct Anneal {  // the arguments every stage of one run has in common, and its host staging
  const double* H_lik;
  int32_t L;
  double eps;
  uint64_t seed;
  int64_t chain_offset;
  double* accept_trace;  // [stages] or NULL
  std::vector<long long> acc;
  std::vector<double> mass, Lm, Mi;
};

// the opening: the per-chain buffers, log weights of zero, and the starting positions in trj.w: theta0, or draws from the prior
int anneal_open(rmhmc_ctx* ctx, const Anneal& a, const double* theta0) {
  ctx->chains_ready = false;
  RC(ais_buffers(ctx));
  HIPCK(hipMemsetAsync(ctx->d_ais_logw, 0, sizeof(double) * ctx->n, ctx->stream));
  if (theta0) return upload_vec(ctx, ctx->batch.ch.trj.w, theta0);
  launch_ais_prior(ctx, a.seed, a.chain_offset, ctx->batch.ch.trj.w, ctx->DP);
  return RMHMC_OK;
}

// the mass bk H_lik + I / alpha of a stage that installs one; a refusal - a matrix that is not finite or not positive definite - keeps
// the previous mass.  Synchronises.
int anneal_mass(rmhmc_ctx* ctx, Anneal& a, double bk) {
  const char* why = "";
  if (ais_stage_mass_images(bk, a.H_lik, ctx->D, ctx->DP, ctx->dd.inv_alpha, a.mass, a.Lm, a.Mi, &why) != RMHMC_OK) return RMHMC_OK;
  return install_mass_images(ctx, a.Lm, a.Mi);
}

// The tail of stage k at temperature bk, from the positions in trj.w: the initial record (which, with logw, adds dbeta loglik to it),
// stage_len tempered iterations under the key seed + 1 + k, and the stage's entry of the acceptance trace.
int anneal_stage(rmhmc_ctx* ctx, Anneal& a, int32_t k, double bk, int64_t stage_len, double* logw, double dbeta) {
  RC(tphmc_init_dev(ctx, bk, logw, dbeta));
  Run run{TPHMC, a.L, 0, a.eps, a.seed + 1 + (uint64_t)k, a.chain_offset, nullptr};
  run.beta = bk;
  RC(hmc_sample_run(ctx, run, stage_len, 0, nullptr, nullptr));  // (no sample buffer: the positions stay in the records)
  if (a.accept_trace) {
    a.acc.resize(ctx->n);
    RC(download(ctx, a.acc.data(), ctx->batch.ch.accepted, ctx->n));
    RC(sync(ctx));
    a.accept_trace[k] = adapt_accept((const int64_t*)a.acc.data(), (int64_t)ctx->n, stage_len);
  }
  return RMHMC_OK;
}

// the weight summary: the partial of the log weights through d_part (device, [5]) into part (host, [5]), and what ais_finish makes of
// it (every output may be NULL); synchronises
int anneal_weights(rmhmc_ctx* ctx, double* d_part, double part[5], double* log_mean_w, double* se, double* ess) {
  RC(ais_partial(ctx, ctx->d_ais_logw, ctx->n, d_part));
  RC(download(ctx, part, (const double*)d_part, (size_t)5));
  RC(sync(ctx));
  const double* parts[1] = {part};
  return ais_finish(parts, 1, nullptr, log_mean_w, se, ess, nullptr, nullptr);
}

}  // namespace

extern "C" {

int rmhmc_tphmc_transition(rmhmc_ctx* ctx, double* w, const double* z, const double* u_len, const double* u_acc, int32_t L, double eps,
                           int32_t* accepted_out, int32_t* nsteps_out, double* H_cur_out, double* H_prop_out, double* w_prop_out,
                           double* p_prop_out, int32_t* status_out, double beta, double* loglik0_out, double* loglik_out) {
  NEED_DATA(ctx);
  if (!w || !z || !u_len || !u_acc || L < 1) return fail(ctx, RMHMC_ERR_INVALID, "tphmc_transition: null pointer or L < 1");
  if (!ais_beta_ok(beta)) return fail(ctx, RMHMC_ERR_INVALID, "tphmc_transition: beta must be finite and >= 0");
  if (!ctx->have_mass) return fail(ctx, RMHMC_ERR_INVALID, "tphmc_transition: rmhmc_phmc_set_mass has not been called");
  return hmc_transition_body(ctx, TPHMC, w, z, u_len, u_acc, L, eps, accepted_out, nsteps_out, H_cur_out, H_prop_out, w_prop_out, p_prop_out, status_out,
                             beta, loglik0_out, loglik_out);
}

int rmhmc_tphmc_sample_to(rmhmc_ctx* ctx, int64_t n_iter, int64_t burn_in, int32_t L, double eps, uint64_t seed, int64_t chain_offset,
                          const double* theta0, const rmhmc_out* out, int64_t* accept_out, int64_t* steps_out, double* seconds_out, double beta,
                          double* loglik0_out, double* loglik_out) {
  NEED_DATA(ctx);
  RC(out_check(ctx, "tphmc_sample_to", out));
  return tphmc_sample_body(ctx, "tphmc_sample_to", n_iter, burn_in, L, eps, seed, chain_offset, theta0, *out, accept_out, steps_out, seconds_out, beta,
                           loglik0_out, loglik_out);
}

int rmhmc_ais_prior(rmhmc_ctx* ctx, uint64_t seed, int64_t chain_offset, double* theta_out) {
  if (!ctx || !theta_out) return fail(ctx, RMHMC_ERR_INVALID, "ais_prior: need a context and theta_out");
  HIPCK(hipSetDevice(ctx->device));
  const size_t nd = (size_t)ctx->n * ctx->D;
  CallMem mem(ctx);
  double* d_th = nullptr;
  RC(mem.alloc(&d_th, sizeof(double) * nd));
  launch_ais_prior(ctx, seed, chain_offset, d_th, ctx->D);
  HIPCK(hipGetLastError());
  RC(download(ctx, theta_out, d_th, nd));
  return sync(ctx);
}

int rmhmc_ais_partial_dev(rmhmc_ctx* ctx, const double* logw_dev, int64_t n, double* partial_dev) {
  if (!ctx || !logw_dev || !partial_dev || n < 1) return fail(ctx, RMHMC_ERR_INVALID, "ais_partial_dev: need logw, a partial and n >= 1");
  HIPCK(hipSetDevice(ctx->device));
  return ais_partial(ctx, logw_dev, (size_t)n, partial_dev);
}

int rmhmc_ais_finish(const double* const* partials, int32_t k, double* merged, double* log_mean_w, double* se, double* weight_ess, int64_t* m_out,
                     int64_t* n_nan_out) {
  const int rc = ais_finish(partials, k, merged, log_mean_w, se, weight_ess, m_out, n_nan_out);
  return rc == RMHMC_OK ? rc : fail(nullptr, rc, "ais_finish: need k >= 1 and no NULL partial");
}

int rmhmc_ais_run(rmhmc_ctx* ctx, const double* theta0, double beta0, int32_t T, const double* beta, const int64_t* stage_len,
                  const int32_t* stage_mass, const double* H_lik, int32_t L, double eps, uint64_t seed, int64_t chain_offset, double* logw_out,
                  double* theta_out, double* accept_trace, double* partial_out, double* seconds_out) {
  NEED_DATA(ctx);
  const auto t_start = std::chrono::steady_clock::now();
  if (const char* why = ais_check_run(theta0 != nullptr, beta0, T, beta, stage_len, stage_mass, H_lik != nullptr, L))
    return fail(ctx, RMHMC_ERR_INVALID, std::string("ais_run: ") + why);
  if (!ctx->have_mass) return fail(ctx, RMHMC_ERR_INVALID, "ais_run: rmhmc_phmc_set_mass has not been called");
  const size_t n = ctx->n;
  Group& g = ctx->batch;
  Anneal a{H_lik, L, eps, seed, chain_offset, accept_trace};
  RC(anneal_open(ctx, a, theta0));
  double prev = beta0;
  for (int32_t k = 0; k < T; ++k) {
    if (stage_mass && stage_mass[k]) RC(anneal_mass(ctx, a, beta[k]));
    // the last positions of the previous stage are the current points of its chains
    if (k > 0) HIPCK(hipMemcpyAsync(g.ch.trj.w, g.ch.cur.w, sizeof(double) * n * ctx->DP, hipMemcpyDeviceToDevice, ctx->stream));
    RC(anneal_stage(ctx, a, k, beta[k], stage_len[k], ctx->d_ais_logw, beta[k] - prev));
    prev = beta[k];
  }
  if (logw_out) RC(download(ctx, logw_out, ctx->d_ais_logw, n));
  if (theta_out) RC(download_vec(ctx, theta_out, g.ch.cur.w));
  CallMem mem(ctx);
  if (partial_out) {
    double* d_part = nullptr;
    RC(mem.alloc(&d_part, sizeof(double) * 5));
    RC(anneal_weights(ctx, d_part, partial_out, nullptr, nullptr, nullptr));
  }
  RC(sync(ctx));
  if (seconds_out) *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
  return RMHMC_OK;
}

}  // extern "C"

// ---- posterior predictive probabilities of new rows (include/rmhmc_pred.h, pred.h, pred.hip.h) -----------------------------------------------
namespace {

// draws [N][D] (device), xnew [R][D] and tnew [R] | NULL (host, checked) -> the partial [4][R] (device); synchronises
int pred_partial(rmhmc_ctx* ctx, const double* d_w, size_t N, int D, const double* xnew, const double* tnew, size_t R, double* d_partial) {
  const pred_plan_t pl = pred_plan((int64_t)N, (int64_t)R, D);
  CallMem mem(ctx);
  double* rec = nullptr;
  RC(mem.alloc(&rec, (size_t)pl.scratch_bytes));
  double* cnt = rec + pl.rec_doubles;
  double* d_x = cnt + pl.cnt_doubles;
  double* d_t = d_x + R * (size_t)D;
  unsigned char* valid = (unsigned char*)(d_t + R);
  const int rc = [&]() -> int {
    RC(upload(ctx, d_x, xnew, R * (size_t)D));
    if (tnew) RC(upload(ctx, d_t, tnew, R));
    const dim3 grid((unsigned)pl.row_tiles, (unsigned)pl.nblocks);
    const double* t_arg = tnew ? d_t : nullptr;
    launch(ctx, "pred", [&](hipStream_t st) {
      hipLaunchKernelGGL(k_pred_valid, dim3((unsigned)pl.vblocks), dim3(256), 0, st, d_w, N, D, (size_t)pl.draws_per_vblock, valid, cnt);
      KS_SWITCH(pl.ksteps, hipLaunchKernelGGL(k_pred_main<KS_>, grid, dim3(64 * PRED_WAVES), 0, st, d_w, N, D, (size_t)pl.draws_per_block, valid, d_x,
                                              t_arg, R, rec));
      hipLaunchKernelGGL(k_pred_fin, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, st, rec, (size_t)pl.nblocks, cnt, (size_t)pl.vblocks, R,
                         tnew ? 1 : 0, d_partial);
    });
    HIPCK(hipGetLastError());
    return RMHMC_OK;
  }();
  return sync_after(ctx, rc);
}

}  // namespace

extern "C" {

int rmhmc_pred_partial_dev(rmhmc_ctx* ctx, const double* samples_dev, int64_t n, int64_t S, int32_t D, const double* xnew, const double* tnew,
                           int64_t R, double* partial_dev) {
  if (!ctx || !samples_dev || !xnew || !partial_dev || n < 1 || S < 1 || D < 1 || R < 1 || n > INT64_MAX / S || R > INT64_MAX / 4 / D ||
      (R + PRED_ROW_TILE - 1) / PRED_ROW_TILE > 0x7fffffffLL)
    return fail(ctx, RMHMC_ERR_INVALID, "pred_partial_dev: need samples, xnew, a partial, n >= 1, S >= 1, D >= 1, R >= 1");
  if (D > PRED_MAX_D) return fail(ctx, RMHMC_ERR_UNSUPPORTED, "pred_partial_dev: D <= 256");
  if (const char* why = pred_check_rows(xnew, tnew, R, D)) return fail(ctx, RMHMC_ERR_INVALID, std::string("pred_partial_dev: ") + why);
  HIPCK(hipSetDevice(ctx->device));
  return pred_partial(ctx, samples_dev, (size_t)n * (size_t)S, D, xnew, tnew, (size_t)R, partial_dev);
}

int rmhmc_pred_finish(const double* const* partials, int32_t k, int64_t R, double* merged, double* prob, double* pvar, double* lpd,
                      double* lpd_total, int64_t* draws_used) {
  const int rc = pred_finish(partials, k, R, merged, prob, pvar, lpd, lpd_total, draws_used);
  return rc == RMHMC_OK ? rc : fail(nullptr, rc, rc == RMHMC_ERR_NOMEM ? "pred_finish: out of memory" : "pred_finish: need k >= 1, R >= 1 and no NULL partial");
}

}  // extern "C"

// ---- leave-one-out cross-validation: PSIS-LOO and WAIC (include/rmhmc_loo.h, loo.h, loo.hip.h) ---------------------------------------------
namespace {

// The device buffers of one block of C <= 64 columns over N draws, carved out of one allocation (base nullptr: sizes only).
// which: 1 the log-likelihood, 2 a reduction, 4 the split, 8 the fit, 16 the select, 32 ll itself
struct LooBufs {
  double *x = nullptr, *t = nullptr, *vcnt = nullptr, *rec = nullptr, *partial = nullptr, *cut = nullptr, *lmin = nullptr, *tail = nullptr,
         *sorted = nullptr, *body = nullptr, *fit = nullptr, *hist = nullptr, *ll = nullptr;
  long long *tail_len = nullptr, *counts = nullptr;
  unsigned long long *fill = nullptr;
  QuantScratch q{nullptr, nullptr, nullptr};
  unsigned char* valid = nullptr;
  size_t bytes = 0;
  template <typename T>
  void take(char* base, T*& p, size_t count) {
    bytes = (bytes + 15) & ~(size_t)15;
    p = base ? (T*)(base + bytes) : nullptr;
    bytes += count * sizeof(T);
  }
  void carve(char* base, int which, size_t N, int D, int C, size_t stride, const loo_plan_t& pl) {
    bytes = 0;
    const size_t c = (size_t)C;
    if (which & 32) take(base, ll, N * c);
    if (which & 1) { take(base, x, c * (size_t)D); take(base, t, c); take(base, vcnt, (size_t)pl.vblocks); take(base, valid, N); }
    if (which & 2) { take(base, rec, (size_t)pl.rblocks * LOO_REC * LOO_MAX_COLS); take(base, partial, 5 * c); }
    if (which & (4 | 8)) { take(base, cut, c); take(base, lmin, c); take(base, tail_len, c); take(base, counts, 2 * c); }
    if (which & 4) { take(base, fill, c); take(base, body, 2 * c); }
    if (which & 32) take(base, tail, c * stride);  // (the single calls take the caller's)
    if (which & 8) { take(base, sorted, c * stride); take(base, fit, 4 * c); }
    if (which & 16) { take(base, hist, c * QUANT_BINS); take(base, q.cnt, c * QUANT_BINS); take(base, q.prefix, c); take(base, q.rep, c); }
  }
  int alloc(rmhmc_ctx*, CallMem& mem, int which, size_t N, int D, int C, size_t stride, const loo_plan_t& pl) {
    carve(nullptr, which, N, D, C, stride, pl);
    char* base = nullptr;
    RC(mem.alloc(&base, bytes));
    carve(base, which, N, D, C, stride, pl);
    return RMHMC_OK;
  }
};

// draws [N][D] (device), x [C][D] and t [C] (host, checked) -> ll [N][C] (device); queued
int loo_loglik(rmhmc_ctx* ctx, const double* d_w, size_t N, int D, const double* x, const double* t, int C, const loo_plan_t& pl, LooBufs& b,
               double* d_ll) {
  RC(upload(ctx, b.x, x, (size_t)C * (size_t)D));
  RC(upload(ctx, b.t, t, (size_t)C));
  launch(ctx, "loo_loglik", [&](hipStream_t st) {
    hipLaunchKernelGGL(k_pred_valid, dim3((unsigned)pl.vblocks), dim3(256), 0, st, d_w, N, D, (size_t)pl.draws_per_vblock, b.valid, b.vcnt);
    KS_SWITCH(pl.ksteps, hipLaunchKernelGGL(k_loo_loglik<KS_>, dim3((unsigned)pl.lblocks), dim3(256), 0, st, d_w, N, D, b.valid, b.x, b.t, C, d_ll));
  });
  HIPCK(hipGetLastError());
  return RMHMC_OK;
}

// ll [N][C] -> the moments partial [5][C], both device; queued
int loo_moments(rmhmc_ctx* ctx, const double* d_ll, size_t N, int C, const loo_plan_t& pl, LooBufs& b, double* d_partial) {
  launch(ctx, "loo_moments", [&](hipStream_t st) {
    const dim3 grid((unsigned)pl.rblocks);
    const loo_split_args none{};
    hipLaunchKernelGGL(k_loo_reduce<0>, grid, dim3(256), 0, st, d_ll, N, C, (size_t)pl.rows_per_block, (const double*)nullptr, none, b.rec);
    hipLaunchKernelGGL(k_loo_fin<0>, dim3(1), dim3(64), 0, st, b.rec, (size_t)pl.rblocks, C, d_partial, none, (long long*)nullptr, (double*)nullptr);
    hipLaunchKernelGGL(k_loo_reduce<1>, grid, dim3(256), 0, st, d_ll, N, C, (size_t)pl.rows_per_block, (const double*)(d_partial + C), none, b.rec);
    hipLaunchKernelGGL(k_loo_fin<1>, dim3(1), dim3(64), 0, st, b.rec, (size_t)pl.rblocks, C, d_partial, none, (long long*)nullptr, (double*)nullptr);
  });
  HIPCK(hipGetLastError());
  return RMHMC_OK;
}

// cut, lmin, tail_len [C] (host) to the device; the caller keeps them until the stream is idle
int loo_upload_cut(rmhmc_ctx* ctx, const double* cut, const double* lmin, const int64_t* tail_len, int C, LooBufs& b) {
  RC(upload(ctx, b.cut, cut, (size_t)C));
  RC(upload(ctx, b.lmin, lmin, (size_t)C));
  RC(upload(ctx, (int64_t*)b.tail_len, tail_len, (size_t)C));
  return RMHMC_OK;
}

// ll [N][C] and the uploaded cut -> tail [C][stride], counts [2][C], body [2][C], all device; queued
int loo_split(rmhmc_ctx* ctx, const double* d_ll, size_t N, int C, size_t stride, const loo_plan_t& pl, LooBufs& b, double* d_tail,
              long long* d_counts, double* d_body) {
  HIPCK(hipMemsetAsync(b.fill, 0, sizeof(unsigned long long) * (size_t)C, ctx->stream));
  launch(ctx, "loo_split", [&](hipStream_t st) {
    const loo_split_args sp{b.cut, b.lmin, b.tail_len, d_tail, (long long)stride, b.fill};
    hipLaunchKernelGGL(k_loo_reduce<2>, dim3((unsigned)pl.rblocks), dim3(256), 0, st, d_ll, N, C, (size_t)pl.rows_per_block, (const double*)nullptr,
                       sp, b.rec);
    hipLaunchKernelGGL(k_loo_fin<2>, dim3(1), dim3(64), 0, st, b.rec, (size_t)pl.rblocks, C, (double*)nullptr, sp, d_counts, d_body);
  });
  HIPCK(hipGetLastError());
  return RMHMC_OK;
}

// tail [C][stride], counts [2][C] and the uploaded cut -> fit [4][C], all device; queued
int loo_fit(rmhmc_ctx* ctx, const double* d_tail, const long long* d_counts, size_t stride, int C, LooBufs& b, double* d_fit) {
  RC(raise_lds(ctx, k_loo_fit, MAX_LDS));  // per device: set where it is used
  launch(ctx, "loo_fit", [&](hipStream_t st) {
    hipLaunchKernelGGL(k_loo_fit, dim3((unsigned)C), dim3(LOO_FIT_THREADS), LOO_FIT_LDS_BYTES, st, d_tail, d_counts, b.cut, b.lmin, b.tail_len,
                       (long long)stride, C, b.sorted, d_fit);
  });
  HIPCK(hipGetLastError());
  return RMHMC_OK;
}

const char* loo_ll_refusal(const rmhmc_ctx* ctx, const void* ll, int64_t n, int64_t S, int32_t C) {
  if (!ctx || !ll || n < 1 || S < 1 || C < 1 || C > LOO_MAX_COLS || n > INT64_MAX / S || n * S > INT64_MAX / 8 / LOO_MAX_COLS)
    return "need a context, ll, n >= 1, S >= 1 and 1 <= C <= 64";
  return nullptr;
}

// one block of columns of rmhmc_loo_dev: x [C][D], t [C] -> the block's partial [5][C], fit [4][C], body [2][C] on the host
int loo_block(rmhmc_ctx* ctx, const double* d_w, size_t N, int D, const double* x, const double* t, int C, size_t stride, const loo_plan_t& pl,
              LooBufs& b, CallMem& mem, double* partial, double* fit, double* body) {
  const size_t c = (size_t)C;
  RC(sync_after(ctx, [&]() -> int {
    RC(loo_loglik(ctx, d_w, N, D, x, t, C, pl, b, b.ll));
    RC(loo_moments(ctx, b.ll, N, C, pl, b, b.partial));
    return download(ctx, partial, b.partial, 5 * c);
  }()));
  std::vector<int64_t> m(c), tl(c), rank(c);
  for (size_t i = 0; i < c; ++i) m[i] = (int64_t)partial[i];
  const int rp = loo_plan(m.data(), C, tl.data(), rank.data());
  if (rp != RMHMC_OK) return fail(ctx, rp, "loo_dev: a column's tail is longer than 16384 draws (more than 29 826 161 finite draws)");
  std::vector<uint64_t> prefix(c, 0);
  std::vector<double> hist(c * QUANT_BINS), cut(c, NAN);
  bool any = false;
  for (size_t i = 0; i < c; ++i) any = any || rank[i] >= 0;
  for (int round = 0; any && round < 8; ++round) {
    RC(sync_after(ctx, [&]() -> int {
      RC(launch_quant_hist(ctx, b.ll, (long long)N, C, round, prefix.data(), 1, b.hist, mem, &b.q));
      return download(ctx, hist.data(), b.hist, hist.size());
    }()));
    const double* one = hist.data();
    const int rs = quant_step(&one, 1, C, 1, round, prefix.data(), rank.data());
    if (rs != RMHMC_OK) return fail(ctx, rs, "loo_dev: a round's histogram does not continue the previous round");
  }
  for (size_t i = 0; i < c; ++i)
    if (tl[i] >= 5) cut[i] = quant_unkey(prefix[i]);
  return sync_after(ctx, [&]() -> int {
    RC(loo_upload_cut(ctx, cut.data(), partial + 4 * c, tl.data(), C, b));
    RC(loo_split(ctx, b.ll, N, C, stride, pl, b, b.tail, b.counts, b.body));
    RC(loo_fit(ctx, b.tail, b.counts, stride, C, b, b.fit));
    RC(download(ctx, body, b.body, 2 * c));
    return download(ctx, fit, b.fit, 4 * c);
  }());
}

}  // namespace

extern "C" {

int rmhmc_loo_loglik_dev(rmhmc_ctx* ctx, const double* samples_dev, int64_t n, int64_t S, int32_t D, const double* x, const double* t, int32_t C,
                         double* ll_dev) {
  if (!samples_dev || !x || !t || D < 1) return fail(ctx, RMHMC_ERR_INVALID, "loo_loglik_dev: need samples, x, t and D >= 1");
  if (const char* why = loo_ll_refusal(ctx, ll_dev, n, S, C)) return fail(ctx, RMHMC_ERR_INVALID, std::string("loo_loglik_dev: ") + why);
  if (D > LOO_MAX_D) return fail(ctx, RMHMC_ERR_UNSUPPORTED, "loo_loglik_dev: D <= 256");
  if (const char* why = loo_check_rows(x, t, C, D)) return fail(ctx, RMHMC_ERR_INVALID, std::string("loo_loglik_dev: ") + why);
  const size_t N = (size_t)n * (size_t)S;
  const loo_plan_t pl = loo_kernel_plan((int64_t)N, D);
  if (pl.lblocks > 0x7fffffffLL) return fail(ctx, RMHMC_ERR_UNSUPPORTED, "loo_loglik_dev: too many draws for one launch");
  HIPCK(hipSetDevice(ctx->device));
  CallMem mem(ctx);
  LooBufs b;
  RC(b.alloc(ctx, mem, 1, N, D, C, 1, pl));
  return sync_after(ctx, loo_loglik(ctx, samples_dev, N, D, x, t, C, pl, b, ll_dev));
}

int rmhmc_loo_moments_dev(rmhmc_ctx* ctx, const double* ll_dev, int64_t n, int64_t S, int32_t C, double* partial_dev) {
  if (const char* why = loo_ll_refusal(ctx, ll_dev, n, S, C)) return fail(ctx, RMHMC_ERR_INVALID, std::string("loo_moments_dev: ") + why);
  if (!partial_dev) return fail(ctx, RMHMC_ERR_INVALID, "loo_moments_dev: need a partial");
  const size_t N = (size_t)n * (size_t)S;
  const loo_plan_t pl = loo_kernel_plan((int64_t)N, 1);
  HIPCK(hipSetDevice(ctx->device));
  CallMem mem(ctx);
  LooBufs b;
  RC(b.alloc(ctx, mem, 2, N, 1, C, 1, pl));
  return sync_after(ctx, loo_moments(ctx, ll_dev, N, C, pl, b, partial_dev));
}

int rmhmc_loo_plan(const int64_t* m, int32_t C, int64_t* tail_len, int64_t* rank) {
  const int rc = loo_plan(m, C, tail_len, rank);
  return rc == RMHMC_OK ? rc : fail(nullptr, rc, rc == RMHMC_ERR_UNSUPPORTED ? "loo_plan: a tail longer than 16384 draws (m above 29 826 161)"
                                                                              : "loo_plan: need m >= 0, C >= 1 and no NULL pointer");
}

int rmhmc_loo_split_dev(rmhmc_ctx* ctx, const double* ll_dev, int64_t n, int64_t S, int32_t C, const double* cut, const double* lmin,
                        const int64_t* tail_len, int64_t stride, double* tail_dev, int64_t* counts_dev, double* body_dev) {
  if (const char* why = loo_ll_refusal(ctx, ll_dev, n, S, C)) return fail(ctx, RMHMC_ERR_INVALID, std::string("loo_split_dev: ") + why);
  if (!cut || !lmin || !tail_len || !tail_dev || !counts_dev || !body_dev) return fail(ctx, RMHMC_ERR_INVALID, "loo_split_dev: a NULL pointer");
  if (const char* why = loo_check_tails(tail_len, C, stride)) return fail(ctx, RMHMC_ERR_INVALID, std::string("loo_split_dev: ") + why);
  const size_t N = (size_t)n * (size_t)S;
  const loo_plan_t pl = loo_kernel_plan((int64_t)N, 1);
  HIPCK(hipSetDevice(ctx->device));
  CallMem mem(ctx);
  LooBufs b;
  RC(b.alloc(ctx, mem, 2 | 4, N, 1, C, 0, pl));
  return sync_after(ctx, [&]() -> int {
    RC(loo_upload_cut(ctx, cut, lmin, tail_len, C, b));
    return loo_split(ctx, ll_dev, N, C, (size_t)stride, pl, b, tail_dev, (long long*)counts_dev, body_dev);
  }());
}

int rmhmc_loo_fit_dev(rmhmc_ctx* ctx, const double* tail_dev, const int64_t* counts_dev, const double* cut, const double* lmin,
                      const int64_t* tail_len, int64_t stride, int32_t C, double* fit_dev) {
  if (!ctx || !tail_dev || !counts_dev || !cut || !lmin || !tail_len || !fit_dev || C < 1 || C > LOO_MAX_COLS)
    return fail(ctx, RMHMC_ERR_INVALID, "loo_fit_dev: need a context, 1 <= C <= 64 and no NULL pointer");
  if (const char* why = loo_check_tails(tail_len, C, stride)) return fail(ctx, RMHMC_ERR_INVALID, std::string("loo_fit_dev: ") + why);
  const loo_plan_t pl = loo_kernel_plan(1, 1);
  HIPCK(hipSetDevice(ctx->device));
  CallMem mem(ctx);
  LooBufs b;
  RC(b.alloc(ctx, mem, 8, 1, 1, C, (size_t)stride, pl));
  return sync_after(ctx, [&]() -> int {
    RC(loo_upload_cut(ctx, cut, lmin, tail_len, C, b));
    return loo_fit(ctx, tail_dev, (const long long*)counts_dev, (size_t)stride, C, b, fit_dev);
  }());
}

int rmhmc_loo_finish(const double* const* partials, int32_t k, int64_t C, const double* fit, const double* body, double* merged, double* elpd_loo,
                     double* p_loo, double* pareto_k, double* lppd, double* p_waic, double* elpd_waic, double* totals, int64_t* k_counts,
                     int64_t* draws_used) {
  const int rc = loo_finish(partials, k, C, fit, body, merged, elpd_loo, p_loo, pareto_k, lppd, p_waic, elpd_waic, totals, k_counts, draws_used);
  return rc == RMHMC_OK ? rc : fail(nullptr, rc, rc == RMHMC_ERR_NOMEM ? "loo_finish: out of memory"
                                                                       : "loo_finish: need k >= 1, C >= 1, no NULL partial, and fit and body together");
}

int rmhmc_loo_dev(rmhmc_ctx* ctx, const double* samples_dev, int64_t n, int64_t S, int32_t D, const double* x, const double* t, int64_t R,
                  int32_t cols_per_block, double* partial, double* fit, double* body, double* elpd_loo, double* p_loo, double* pareto_k, double* lppd,
                  double* p_waic, double* elpd_waic, double* totals, int64_t* k_counts, int64_t* draws_used) {
  if (!ctx || !samples_dev || !x || !t || n < 1 || S < 1 || D < 1 || R < 1 || n > INT64_MAX / S || n * S > INT64_MAX / 8 / LOO_MAX_COLS ||
      R > INT64_MAX / 8 / (D > LOO_MAX_D ? D : LOO_MAX_D) || cols_per_block < 0 || cols_per_block > LOO_MAX_COLS)
    return fail(ctx, RMHMC_ERR_INVALID, "loo_dev: need samples, x, t, n >= 1, S >= 1, D >= 1, R >= 1 and 0 <= cols_per_block <= 64");
  if (D > LOO_MAX_D) return fail(ctx, RMHMC_ERR_UNSUPPORTED, "loo_dev: D <= 256");
  if (const char* why = loo_check_rows(x, t, R, D)) return fail(ctx, RMHMC_ERR_INVALID, std::string("loo_dev: ") + why);
  const size_t N = (size_t)n * (size_t)S, r = (size_t)R;
  const loo_plan_t pl = loo_kernel_plan((int64_t)N, D);
  if (pl.lblocks > 0x7fffffffLL) return fail(ctx, RMHMC_ERR_UNSUPPORTED, "loo_dev: too many draws for one launch");
  int cb = cols_per_block ? cols_per_block : loo_cols_per_block((int64_t)N);
  if ((size_t)cb > r) cb = (int)r;
  int64_t bound = loo_tail_len((int64_t)N);  // no column's tail is longer: the tail length grows with m <= N
  const size_t stride = (size_t)(bound < 1 ? 1 : bound > LOO_MAX_TAIL ? LOO_MAX_TAIL : bound);
  HIPCK(hipSetDevice(ctx->device));
  CallMem mem(ctx);
  LooBufs b;
  RC(b.alloc(ctx, mem, 63, N, D, cb, stride, pl));
  std::vector<double> P(5 * r), F(4 * r), B(2 * r), p((size_t)5 * cb), f((size_t)4 * cb), bd((size_t)2 * cb);
  for (size_t c0 = 0; c0 < r; c0 += (size_t)cb) {
    const int C = (int)std::min<size_t>((size_t)cb, r - c0);
    RC(loo_block(ctx, samples_dev, N, D, x + c0 * (size_t)D, t + c0, C, stride, pl, b, mem, p.data(), f.data(), bd.data()));
    for (int q = 0; q < 5; ++q)
      for (int c = 0; c < C; ++c) {
        P[(size_t)q * r + c0 + c] = p[(size_t)q * C + c];
        if (q < 4) F[(size_t)q * r + c0 + c] = f[(size_t)q * C + c];
        if (q < 2) B[(size_t)q * r + c0 + c] = bd[(size_t)q * C + c];
      }
  }
  const double* one = P.data();
  RC(rmhmc_loo_finish(&one, 1, R, F.data(), B.data(), nullptr, elpd_loo, p_loo, pareto_k, lppd, p_waic, elpd_waic, totals, k_counts, draws_used));
  if (partial) std::copy(P.begin(), P.end(), partial);
  if (fit) std::copy(F.begin(), F.end(), fit);
  if (body) std::copy(B.begin(), B.end(), body);
  return RMHMC_OK;
}

}  // extern "C"

// ---- the evidence by adaptive sequential Monte Carlo (include/rmhmc_smc.h, smc.h, smc.hip.h) ------------------------------------------------
namespace {

// doubles of scratch that smc_cess needs for J candidates: blk [nb][NQ], sums [nb][NQ][2]
size_t smc_cess_scratch(size_t n, int J) {
  int64_t nb, pb;
  ais_plan((int64_t)n, &nb, &pb);
  const int JT = J <= 1 ? 1 : J <= 4 ? 4 : J <= 16 ? 16 : 32;
  return 3 * (size_t)nb * (size_t)(1 + 2 * JT);
}
// the conditional-ESS partial of (logw, ll) [n] at the J candidates delta (checked) -> d_partial [2 + 4 J], all in device memory; d_scr:
// smc_cess_scratch doubles, or nullptr: the call's own; synchronises, unless the caller owns the scratch and waits for the stream itself
int smc_cess(rmhmc_ctx* ctx, const double* d_lw, const double* d_ll, size_t n, int J, const double* delta, double* d_partial, double* d_scr = nullptr) {
  const bool wait = d_scr == nullptr;
  int64_t nb, pb;
  ais_plan((int64_t)n, &nb, &pb);
  const int JT = J <= 1 ? 1 : J <= 4 ? 4 : J <= 16 ? 16 : 32;
  const int NQ = 1 + 2 * JT;
  SmcDeltas dl;
  for (int j = 0; j < RMHMC_SMC_MAX_J; ++j) dl.d[j] = delta[j < J ? j : J - 1];
  CallMem mem(ctx);
  if (!d_scr) RC(mem.alloc(&d_scr, sizeof(double) * smc_cess_scratch(n, J)));
  double* d_blk = d_scr;
  double* d_sums = d_blk + (size_t)nb * NQ;
  launch(ctx, "smc", [&](hipStream_t st) {
    switch (JT) {
#define SMC_CASE(JT_)                                                                                                                        \
  case JT_:                                                                                                                                  \
    hipLaunchKernelGGL(k_smc_cess_max<JT_>, dim3((unsigned)nb), dim3(256), 0, st, d_lw, d_ll, n, (size_t)pb, dl, d_blk);                        \
    hipLaunchKernelGGL(k_smc_cess_sums<JT_>, dim3((unsigned)nb), dim3(256), 0, st, d_lw, d_ll, n, (size_t)pb, dl, (const double*)d_blk, (int)nb, \
                       d_sums);                                                                                                              \
    break
      SMC_CASE(1); SMC_CASE(4); SMC_CASE(16);
      default: SMC_CASE(32);
#undef SMC_CASE
    }
    hipLaunchKernelGGL(k_smc_cess_fin, dim3(1), dim3(128), 0, st, (const double*)d_blk, (const double*)d_sums, (int)nb, NQ, 1 + 2 * J, d_partial);
  });
  const hipError_t e = hipGetLastError();
  const int rs = wait ? sync(ctx) : RMHMC_OK;
  if (e != hipSuccess) return fail(ctx, RMHMC_ERR_RUNTIME, std::string(hipGetErrorString(e)) + " in smc_cess");
  return rs;
}

// the search of include/rmhmc_smc.h section 2 (arguments checked); d_part: device scratch of 2 + 4 RMHMC_SMC_J doubles followed by
// smc_cess_scratch(n, RMHMC_SMC_J) more
int smc_choose_delta(rmhmc_ctx* ctx, const double* d_lw, const double* d_ll, size_t n, double remaining, double rho, double* d_part, double* delta_out,
                     double* frac_out, int32_t* flags_out) {
  smc_search s;
  smc_search_init(&s, remaining, rho);
  double grid[RMHMC_SMC_J], frac[RMHMC_SMC_J], part[2 + 4 * RMHMC_SMC_J];
  const double* parts[1] = {part};
  while (!s.done) {
    smc_search_grid(&s, grid);
    RC(smc_cess(ctx, d_lw, d_ll, n, RMHMC_SMC_J, grid, d_part, d_part + 2 + 4 * RMHMC_SMC_J));
    RC(download(ctx, part, (const double*)d_part, (size_t)(2 + 4 * RMHMC_SMC_J)));
    RC(sync(ctx));
    (void)smc_cess_finish(parts, 1, RMHMC_SMC_J, nullptr, frac);
    smc_search_step(&s, grid, frac);
  }
  if (delta_out) *delta_out = s.delta;
  if (frac_out) *frac_out = s.frac;
  if (flags_out) *flags_out = s.flags;
  return RMHMC_OK;
}

// wait = false: queued on the stream, for a caller that goes on in it
int smc_reweight(rmhmc_ctx* ctx, double* d_lw, const double* d_ll, size_t n, double delta, bool wait = true) {
  launch(ctx, "smc", [&](hipStream_t st) {
    hipLaunchKernelGGL(k_smc_reweight, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_lw, d_ll, n, delta);
  });
  HIPCK(hipGetLastError());
  return wait ? sync(ctx) : RMHMC_OK;
}

int smc_quantise(rmhmc_ctx* ctx, const double* d_lw, size_t n, double a, uint64_t* d_q, bool wait = true) {
  launch(ctx, "smc", [&](hipStream_t st) {
    hipLaunchKernelGGL(k_smc_quantise, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_lw, n, a, (unsigned long long*)d_q);
  });
  HIPCK(hipGetLastError());
  return wait ? sync(ctx) : RMHMC_OK;
}

// anc of include/rmhmc_smc.h section 4 (1 <= n <= 2^20 checked); a refusal leaves d_anc untouched
int smc_ancestors(rmhmc_ctx* ctx, const uint64_t* d_q, size_t n, uint32_t U, int32_t* d_anc) {
  int64_t nb, pb;
  smc_scan_plan((int64_t)n, &nb, &pb);
  CallMem mem(ctx);
  unsigned long long* d_C = nullptr;  // C [n], blk_sum [nb], blk_bad [nb], off [nb], head [2]
  RC(mem.alloc(&d_C, sizeof(unsigned long long) * (n + 3 * (size_t)nb + 2)));
  unsigned long long *d_sum = d_C + n, *d_bad = d_sum + nb, *d_off = d_bad + nb, *d_head = d_off + nb;
  launch(ctx, "smc", [&](hipStream_t st) {
    hipLaunchKernelGGL(k_smc_scan_blocks, dim3((unsigned)nb), dim3(256), 0, st, (const unsigned long long*)d_q, n, d_C, d_sum, d_bad);
    hipLaunchKernelGGL(k_smc_scan_offsets, dim3(1), dim3(256), 0, st, (const unsigned long long*)d_sum, (const unsigned long long*)d_bad, (int)nb, d_off,
                       d_head);
  });
  HIPCK(hipGetLastError());
  unsigned long long head[2] = {0ull, 0ull};
  RC(download(ctx, head, (const unsigned long long*)d_head, (size_t)2));
  RC(sync(ctx));
  if (head[1] != 0ull) return fail(ctx, RMHMC_ERR_INVALID, "smc_ancestors: an entry of q is above 2^40");
  if (head[0] == 0ull) return fail(ctx, RMHMC_ERR_INVALID, "smc_ancestors: every q is 0 (Q = 0)");
  launch(ctx, "smc", [&](hipStream_t st) {
    hipLaunchKernelGGL(k_smc_ancestors, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const unsigned long long*)d_C, (const unsigned long long*)d_off,
                       n, (unsigned int)U, head[0], (int*)d_anc);
  });
  HIPCK(hipGetLastError());
  return sync(ctx);
}

}  // namespace

extern "C" {

int rmhmc_smc_cess_dev(rmhmc_ctx* ctx, const double* logw_dev, const double* ll_dev, int64_t n, int32_t J, const double* delta, double* partial_dev) {
  if (!ctx || !logw_dev || !ll_dev || !partial_dev) return fail(ctx, RMHMC_ERR_INVALID, "smc_cess_dev: need a context, logw, ll and a partial");
  if (const char* why = smc_check_cess(n, J, delta)) return fail(ctx, RMHMC_ERR_INVALID, std::string("smc_cess_dev: ") + why);
  HIPCK(hipSetDevice(ctx->device));
  return smc_cess(ctx, logw_dev, ll_dev, (size_t)n, J, delta, partial_dev);
}

int rmhmc_smc_cess_finish(const double* const* partials, int32_t k, int32_t J, double* merged, double* frac) {
  const int rc = smc_cess_finish(partials, k, J, merged, frac);
  return rc == RMHMC_OK ? rc : fail(nullptr, rc, "smc_cess_finish: need k >= 1, 1 <= J <= 32 and no NULL partial");
}

int rmhmc_smc_choose_delta_dev(rmhmc_ctx* ctx, const double* logw_dev, const double* ll_dev, int64_t n, double remaining, double rho, double* delta_out,
                               double* frac_out, int32_t* flags_out) {
  if (!ctx || !logw_dev || !ll_dev) return fail(ctx, RMHMC_ERR_INVALID, "smc_choose_delta_dev: need a context, logw and ll");
  if (const char* why = smc_check_search(n, remaining, rho)) return fail(ctx, RMHMC_ERR_INVALID, std::string("smc_choose_delta_dev: ") + why);
  HIPCK(hipSetDevice(ctx->device));
  CallMem mem(ctx);
  double* d_part = nullptr;
  RC(mem.alloc(&d_part, sizeof(double) * (2 + 4 * RMHMC_SMC_J + smc_cess_scratch((size_t)n, RMHMC_SMC_J))));
  return smc_choose_delta(ctx, logw_dev, ll_dev, (size_t)n, remaining, rho, d_part, delta_out, frac_out, flags_out);
}

int rmhmc_smc_reweight_dev(rmhmc_ctx* ctx, double* logw_dev, const double* ll_dev, int64_t n, double delta) {
  if (!ctx || !logw_dev || !ll_dev || n < 1 || !std::isfinite(delta))
    return fail(ctx, RMHMC_ERR_INVALID, "smc_reweight_dev: need a context, logw, ll, n >= 1 and a finite delta");
  HIPCK(hipSetDevice(ctx->device));
  return smc_reweight(ctx, logw_dev, ll_dev, (size_t)n, delta);
}

int rmhmc_smc_quantise_dev(rmhmc_ctx* ctx, const double* logw_dev, int64_t n, double a, uint64_t* q_dev) {
  if (!ctx || !logw_dev || !q_dev || n < 1 || a != a) return fail(ctx, RMHMC_ERR_INVALID, "smc_quantise_dev: need a context, logw, q, n >= 1 and a maximum");
  HIPCK(hipSetDevice(ctx->device));
  return smc_quantise(ctx, logw_dev, (size_t)n, a, q_dev);
}

int rmhmc_smc_ancestors_dev(rmhmc_ctx* ctx, const uint64_t* q_dev, int64_t n, uint32_t U, int32_t* anc_dev) {
  if (!ctx || !q_dev || !anc_dev) return fail(ctx, RMHMC_ERR_INVALID, "smc_ancestors_dev: need a context, q and anc");
  if (const int rc = smc_check_ancestors(n))
    return fail(ctx, rc, rc == RMHMC_ERR_UNSUPPORTED ? "smc_ancestors_dev: n <= 2^20" : "smc_ancestors_dev: need n >= 1");
  HIPCK(hipSetDevice(ctx->device));
  return smc_ancestors(ctx, q_dev, (size_t)n, U, anc_dev);
}

int rmhmc_smc_run(rmhmc_ctx* ctx, const double* theta0, double beta0, double rho, double tau, int32_t T_max, int64_t stage_len, int64_t mass_every,
                  const double* H_lik, int32_t L, double eps, uint64_t seed, int64_t chain_offset, int32_t* T_out, double* beta_out, double* cess_out,
                  double* ess_out, int32_t* flags_out, double* accept_trace, double* logw_out, double* theta_out, double* log_z_out, double* se_out,
                  double* partial_out, double* seconds_out) {
  NEED_DATA(ctx);
  const auto t_start = std::chrono::steady_clock::now();
  if (const char* why = smc_check_run(theta0 != nullptr, beta0, rho, tau, T_max, stage_len, mass_every, H_lik != nullptr, L))
    return fail(ctx, RMHMC_ERR_INVALID, std::string("smc_run: ") + why);
  if (!ctx->have_mass) return fail(ctx, RMHMC_ERR_INVALID, "smc_run: rmhmc_phmc_set_mass has not been called");
  if (tau > 0.0 && ctx->n > RMHMC_SMC_MAX_N) return fail(ctx, RMHMC_ERR_UNSUPPORTED, "smc_run: resampling needs n <= 2^20 chains");
  const size_t n = ctx->n;
  Group& g = ctx->batch;
  Anneal a{H_lik, L, eps, seed, chain_offset, accept_trace};
  RC(anneal_open(ctx, a, theta0));
  CallMem mem(ctx);
  double* d_part = nullptr;  // the weight partial [5], the conditional-ESS partial [2 + 4 J] and its scratch, q [n], anc [n]
  const size_t head = 5 + 2 + 4 * RMHMC_SMC_J + smc_cess_scratch(n, RMHMC_SMC_J);
  RC(mem.alloc(&d_part, sizeof(double) * (head + n) + sizeof(int32_t) * n));
  double* d_cess = d_part + 5;
  uint64_t* d_q = (uint64_t*)(d_part + head);
  int32_t* d_anc = (int32_t*)(d_q + n);
  RC(tphmc_init_dev(ctx, beta0, nullptr, 0.0));  // loglik at the start -> d_ais_ll; trj -> cur
  double part[5], log_mean_w = NAN, ess = NAN, se = NAN;
  double beta = beta0, logz_acc = 0.0;
  bool resampled_any = false;
  int32_t k = 0;
  for (; beta < 1.0 && k < T_max; ++k) {
    double delta = 0.0, frac = NAN;
    int32_t flags = 0;
    RC(smc_choose_delta(ctx, ctx->d_ais_logw, ctx->d_ais_ll, n, 1.0 - beta, rho, d_cess, &delta, &frac, &flags));
    const double bk = (flags & RMHMC_SMC_LAST) ? 1.0 : beta + delta;
    RC(smc_reweight(ctx, ctx->d_ais_logw, ctx->d_ais_ll, n, delta, false));
    RC(anneal_weights(ctx, d_part, part, &log_mean_w, &se, &ess));
    if (ess < tau * (double)n) {
      logz_acc += log_mean_w;
      RC(smc_quantise(ctx, ctx->d_ais_logw, n, part[2], d_q, false));
      RC(smc_ancestors(ctx, d_q, n, smc_resample_u(seed, k), d_anc));
      launch(ctx, "smc", [&](hipStream_t st) {
        hipLaunchKernelGGL(k_smc_gather, dim3((unsigned)n), dim3(64), 0, st, (const double*)g.ch.cur.w, g.ch.trj.w, (const int*)d_anc, ctx->DP);
      });
      HIPCK(hipGetLastError());
      HIPCK(hipMemsetAsync(ctx->d_ais_logw, 0, sizeof(double) * n, ctx->stream));
      flags |= RMHMC_SMC_RESAMPLED;
      resampled_any = true;
    } else {
      HIPCK(hipMemcpyAsync(g.ch.trj.w, g.ch.cur.w, sizeof(double) * n * ctx->DP, hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (smc_stage_mass(k, mass_every, flags)) RC(anneal_mass(ctx, a, bk));
    RC(anneal_stage(ctx, a, k, bk, stage_len, nullptr, 0.0));
    if (beta_out) beta_out[k] = bk;
    if (cess_out) cess_out[k] = frac;
    if (ess_out) ess_out[k] = ess;
    if (flags_out) flags_out[k] = flags;
    beta = bk;
  }
  RC(anneal_weights(ctx, d_part, part, &log_mean_w, &se, &ess));
  if (T_out) *T_out = k;
  if (logw_out) RC(download(ctx, logw_out, (const double*)ctx->d_ais_logw, n));
  if (theta_out) RC(download_vec(ctx, theta_out, g.ch.cur.w));
  RC(sync(ctx));
  if (log_z_out) *log_z_out = beta < 1.0 ? NAN : logz_acc + log_mean_w;
  if (se_out) *se_out = resampled_any ? NAN : se;
  if (partial_out) std::copy(part, part + 5, partial_out);
  if (seconds_out) *seconds_out = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
  return RMHMC_OK;
}

}  // extern "C"
