"""Chain sharding across the GPUs of one node.

Chains never interact (the reference has exactly one chain, ``rmhmc.py:37-191``), so the path
partitions by chain index: rank r runs chains ``[start_r, end_r)`` on its own GPU with X, t replicated by
its own ``rmhmc_set_data`` (ranks that are not handed the data get it from rank 0 by one broadcast before the
run) and **no collective inside the sampling loop**.  The Philox counters use the
global chain id (``chain_offset``), so every chain draws the same random numbers whatever the number of ranks, and the
arithmetic class - fixed-point or fp64 metric - is chosen from the JOB (``shard_flags``), never from the shard.  What the
samples then depend on is the plan of the context a chain runs in (csrc/plan.h), see "What sharding leaves unchanged"
below.  The single
exchange is the gather at write-out (``torch.distributed``: RCCL over xGMI for the ``nccl`` backend, gloo
in the CPU tests), fed from device memory: the sampler writes its outputs through the ``_dev`` entry points of
include/rmhmc.h into torch tensors in HBM and those tensors are what RCCL sends.  One process per GPU, launched by ``torch.distributed.run``.
The other five samplers shard the same way through the output descriptor of include/rmhmc_out.h (``sampler=``).

What sharding leaves unchanged (tests/test_gpu_batch_invariance.py).  Under one plan a chain's samples and
counters are a function of (data, seed, global chain id, run arguments): bit-identical whatever the size of its batch, its slot and
its neighbours.  The plan of a context follows its own chain count, so a sharded job equals the one-rank job BIT FOR BIT when
every shard's plan equals the one-rank plan in the fields that order a sum or pick a kernel: the stepping path (``fused``,
``medium``, ``hmc_traj``), the row splits ``nsplit`` and ``fsplit``, the int8 k pieces ``ksplit_a`` / ``ksplit_l``, and the
variant of the adaptive Metropolis kernel (``amh_shape``: 1024 chains).  With the default options these move with the chain
count (512 chains for the one-launch step and, with more than 1024 data rows, for ``k_hmc_traj``; 1024 chains for the row ranges
of the fp64 assembly; ``nsplit`` with every 16 chains); the create options ``nsplit_max``, ``fsplit``, ``medium`` and
``hmc_traj_maxn`` pin them.  Otherwise the shards agree with one rank to summation-order rounding per transition (the bounds
the paths hold against each other and against the oracle), and a discrete decision - an accept, a trajectory length - can
differ only where a uniform draw falls within that rounding of its threshold, after which that chain's path is another one.
"""
import os

import numpy as np

from . import _capi
from .experiment import SAMPLERS

# experiment.SAMPLERS key -> (sampler of _capi.SAMPLERS_TO, it assembles a metric: the int8 auto-flag rule applies)
_SHARDED = {"RMHMC": ("rmhmc", True), "HMC": ("hmc", False), "mMALA": ("mmala", True), "AMH": ("amh", False), "IWLS": ("iwls", True),
            "Gibbs": ("gibbs", False)}
assert set(_SHARDED) == set(SAMPLERS)


def shard_flags(sampler, D, n_chains, N, compat=False):
    """The context flags of EVERY shard of a job of ``n_chains`` chains of ``sampler`` (a key of experiment.SAMPLERS) on N x D data:
    the reference's guards for RMHMC with ``compat``, and the int8 metric assembly where the sampler assembles a metric and the JOB
    is large enough for it to pay (_capi.auto_metric_flags).  A function of the job alone: fixed-point or fp64 metric is an accuracy
    class, and it must not change with the number of ranks the job happens to run on."""
    has_metric = _SHARDED[sampler][1]
    flags = _capi.COMPAT if (compat and sampler == "RMHMC") else 0
    return flags | (_capi.auto_metric_flags(D, n_chains, M=N) if has_metric else 0)


def shard_range(n_total, world, rank):
    """Contiguous, balanced partition of chain ids: the first (n_total % world) ranks get one more."""
    base, extra = divmod(int(n_total), int(world))
    start = rank * base + min(rank, extra)
    return start, start + base + (1 if rank < extra else 0)


def _dist():
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        raise RuntimeError("torch.distributed is not initialised (launch with torch.distributed.run)")
    return dist


def _gather_rows(local, counts):
    """Gather variable-length leading-dimension TENSORS to rank 0, padding to the longest shard.  `local` lives where the
    collective runs: in HBM for the nccl backend (RCCL moves it over xGMI straight from the buffer the sampler wrote - no host
    bounce), in host memory for gloo.  Rank 0 gets one tensor on the same device, other ranks None."""
    import torch
    dist = _dist()
    rank, world = dist.get_rank(), dist.get_world_size()
    mx = max(counts)
    if local.shape[0] != mx:
        pad = torch.zeros((mx,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
        pad[: local.shape[0]] = local
        local = pad
    local = local.contiguous()
    bufs = [torch.empty_like(local) for _ in range(world)] if rank == 0 else None
    dist.gather(local, bufs, dst=0)
    if rank != 0:
        return None
    return torch.cat([b[: counts[r]] for r, b in enumerate(bufs)], dim=0)


def _replicate_data(XX, t, device):
    """Every rank needs (XX, t) for its own rmhmc_set_data.  Ranks that pass None receive rank 0's arrays by one broadcast (5 MB at
    config 4) before the run; when every rank has the data already (synthetic recipes) nothing is sent."""
    import torch
    dist = _dist()
    have = torch.tensor([0 if XX is None else 1], dtype=torch.int64, device=device)
    dist.all_reduce(have, op=dist.ReduceOp.MIN)
    if int(have.item()) == 1:
        return np.ascontiguousarray(XX, dtype=np.float64), np.ascontiguousarray(t, dtype=np.float64).reshape(-1)
    shape = torch.zeros(2, dtype=torch.int64, device=device)
    if dist.get_rank() == 0:
        if XX is None:
            raise ValueError("rank 0 must hold the data")
        XX = np.ascontiguousarray(XX, dtype=np.float64)
        shape = torch.tensor(XX.shape, dtype=torch.int64, device=device)
    dist.broadcast(shape, src=0)
    N, D = int(shape[0]), int(shape[1])
    buf = torch.empty(N * D + N, dtype=torch.float64, device=device)
    if dist.get_rank() == 0:
        buf.copy_(torch.from_numpy(np.concatenate([XX.ravel(), np.asarray(t, dtype=np.float64).ravel()])))
    dist.broadcast(buf, src=0)
    h = buf.cpu().numpy()
    return np.ascontiguousarray(h[: N * D].reshape(N, D)), np.ascontiguousarray(h[N * D:])


def nanmin_rows(ess):
    """min over the dimensions of a (chains, D) ESS tensor ignoring NaN entries (a constant coordinate has no ESS); a chain whose ESS is NaN
    in EVERY dimension (a constant or diverged chain) gets NaN - not +inf, which would read as a perfect chain in any sum or mean"""
    import torch
    m = torch.nan_to_num(ess, nan=float("inf")).amin(dim=1, keepdim=True)
    m[torch.isinf(m)] = float("nan")
    return m


def sample_sharded(XX, t, n_chains, NumOfIterations=6000, BurnIn=1000, NumOfLeapFrogSteps=6, StepSize=0.5,
                   NumOfNewtonSteps=4, *, seed=0, compat=True, theta0=None, alpha=100.0, gather="samples", lib=None, options=None,
                   sampler="RMHMC", sampler_args=None, diagnostics=False, max_lag=None, quantiles=None):
    """Run ``n_chains`` chains sharded over the ranks of the initialised process group.

    The samples and counters are those of one rank bit for bit when every shard's plan equals the one-rank plan in the stepping path,
    ``nsplit``, ``fsplit``, the int8 k pieces and ``amh_shape`` (module docstring; the create options in ``options`` can pin them), and
    agree with one rank to summation-order rounding per transition otherwise.  The context flags - the int8 or the fp64 metric among
    them - are those of the whole job on every rank (``shard_flags``).

    gather="samples": rank 0 returns (samples [n_chains,S,D], seconds, info); other ranks return None.
    gather="summary": only per-chain posterior mean / variance / min-ESS travel (config 4 at S=5000 would be
    168 GB of raw samples); rank 0 returns (summary dict, seconds, info).  min_ess of a chain whose ESS is NaN in
    every dimension (a constant or diverged chain) is NaN, not a number.
    XX, t may be None on ranks other than 0: they are broadcast once from rank 0.
    ``lib`` is the loaded C-ABI library (default: the HIP library; the CPU tests inject the oracle); ``options``: tuning options of
    include/rmhmc.h for the contexts.
    ``sampler``: a key of experiment.SAMPLERS.  "RMHMC" (the default) runs as described above.  Any other runs NumOfIterations / BurnIn
    iterations through its *_sample_to entry point (include/rmhmc_out.h; HIP library only); NumOfLeapFrogSteps, StepSize,
    NumOfNewtonSteps and ``compat`` are RMHMC's and do not apply: ``sampler_args`` carries the sampler's own run arguments as
    _capi.Context.sample_to takes them (L, eps for HMC; eps for mMALA; compat for IWLS), its defaults otherwise.  ``info`` then holds the
    sampler's own counters.  The int8 metric assembly is chosen as for RMHMC, from the job's chain count, where the sampler assembles a
    metric (mMALA, IWLS).
    ``diagnostics=True`` (every sampler, both gather modes; HIP library only): ``info`` gains rhat, ess_pooled, pairs and chains_used (D,),
    the split R-hat and the pooled ESS across ALL n_chains chains (include/rmhmc_diag.h; ``max_lag`` as there).  Every rank reduces the
    samples of its shard to a partial on its GPU - an empty shard contributes the identity - and the partials, a few KB each, are
    gathered to rank 0 and merged there in rank order.  "RMHMC" then runs through rmhmc_sample_to as the other samplers do, which by the
    contract of include/rmhmc_out.h gives the same samples and counters.  GIVEN the samples, the merged result does not depend on the
    number of ranks beyond rounding (the merge is exact arithmetic only for the counts); whether the samples themselves do is the
    statement above.
    ``quantiles=probs`` (every sampler, both gather modes; HIP library only): ``info`` gains quantiles (Q, D) and quantile_draws (D,), the
    exact posterior quantiles over ALL n_chains chains (include/rmhmc_quant.h).  Every rank counts the histogram of a round on its GPU - an
    empty shard contributes the identity without a launch -, one all_reduce(SUM) per round merges them, and every rank takes the same step
    on the sum; no sample leaves its GPU.  Counts add exactly, so GIVEN the samples the quantiles are the same to the bit for any number of
    ranks: a statement about the merge, not about the samples.
    """
    if sampler not in _SHARDED:   # (before any collective: every rank raises on its own)
        raise ValueError("unknown sampler %r: one of %s" % (sampler, sorted(_SHARDED)))
    if sampler == "RMHMC" and sampler_args:
        raise ValueError("RMHMC takes its run arguments by name (NumOfLeapFrogSteps, StepSize, NumOfNewtonSteps), not in sampler_args")
    if diagnostics:
        _capi.diag_lags(NumOfIterations - BurnIn, max_lag)
        if gather not in ("samples", "summary"):
            raise ValueError('gather must be "samples" or "summary"')
    if quantiles is not None:
        quantiles = _capi.quant_probs(quantiles)
        if gather not in ("samples", "summary"):
            raise ValueError('gather must be "samples" or "summary"')
    if sampler != "RMHMC":
        # everything a rank could raise on its own later: a rank with an empty shard would otherwise wait in a collective for one that raised
        key = _SHARDED[sampler][0]
        if gather not in ("samples", "summary"):
            raise ValueError('gather must be "samples" or "summary"')
        allowed = [k for k in _capi.SAMPLER_ARGS[key] if k != "theta0"]
        bad = sorted(set(sampler_args or {}) - set(allowed))
        if bad:
            raise ValueError("sampler_args of %s may hold %s, not %s" % (sampler, allowed or "nothing", bad))
        if theta0 is not None and "theta0" not in _capi.SAMPLER_ARGS[key]:
            raise ValueError("the %s sampler has no theta0" % sampler)
    import torch as _t
    dist = _dist()
    rank, world = dist.get_rank(), dist.get_world_size()
    backend = dist.get_backend()
    local_rank = int(os.environ.get("LOCAL_RANK", rank))
    lib = lib if lib is not None else _capi.load_hip_library()
    if sampler != "RMHMC" and not lib.has_out:   # (before the first collective as well)
        raise _capi.RmhmcError(-4, "%s does not export the output descriptor (include/rmhmc_out.h): only RMHMC can be sharded" % lib.path)
    if diagnostics and not (lib.has_out and lib.has_diag):
        raise _capi.RmhmcError(-4, "%s does not export the cross-chain diagnostics (include/rmhmc_diag.h, include/rmhmc_out.h)" % lib.path)
    if quantiles is not None and not (lib.has_out and lib.has_quant):
        raise _capi.RmhmcError(-4, "%s does not export the posterior quantiles (include/rmhmc_quant.h, include/rmhmc_out.h)" % lib.path)
    # where the collective runs (HBM for RCCL, host memory for gloo) and where the sampler writes its outputs: the HIP library always
    # writes through device pointers of its own GPU, whatever the backend; with gloo those tensors take one hop to the host first
    cdev = _t.device("cuda", local_rank) if backend == "nccl" else _t.device("cpu")
    gpu = (local_rank % max(1, _t.cuda.device_count())) if lib.on_gpu else 0
    odev = _t.device("cuda", gpu) if lib.on_gpu else _t.device("cpu")
    XX, t = _replicate_data(XX, t, cdev)
    N, D = XX.shape
    start, end = shard_range(n_chains, world, rank)
    counts = [shard_range(n_chains, world, r)[1] - shard_range(n_chains, world, r)[0] for r in range(world)]
    n_local = end - start
    S = NumOfIterations - BurnIn
    if sampler != "RMHMC":
        return _sharded_to(sampler, dict(sampler_args or {}), XX, t, n_chains, NumOfIterations, BurnIn, seed, theta0, alpha, gather, lib,
                           options, gpu, odev, cdev, start, end, counts, diagnostics=diagnostics, max_lag=max_lag, quantiles=quantiles)
    if diagnostics or quantiles is not None:   # the same run through rmhmc_sample_to: its samples stay where the partial is computed
        args = dict(L=NumOfLeapFrogSteps, eps=StepSize, K=NumOfNewtonSteps)
        return _sharded_to(sampler, args, XX, t, n_chains, NumOfIterations, BurnIn, seed, theta0, alpha, gather, lib, options, gpu, odev,
                           cdev, start, end, counts, diagnostics=diagnostics, max_lag=max_lag, compat=compat, quantiles=quantiles)
    if n_local > 0:
        th = None if theta0 is None else np.broadcast_to(theta0, (n_chains, D))[start:end]
        with lib.context(N, D, n_local, flags=shard_flags(sampler, D, n_chains, N, compat), device=gpu, options=options) as ctx:
            ctx.set_data(XX, t, alpha)
            # device-resident write-out (rmhmc_sample_dev / rmhmc_sample_stats_dev): the outputs stay in this rank's HBM
            if gather == "samples":
                smp, acc, steps, secs = ctx.sample_dev(odev, NumOfIterations, BurnIn, NumOfLeapFrogSteps, StepSize, NumOfNewtonSteps,
                                                       seed=seed, chain_offset=start, theta0=th)
                summ = None
            else:  # reduced on the device: no raw sample leaves the GPU at all
                st = ctx.sample_stats_dev(odev, NumOfIterations, BurnIn, NumOfLeapFrogSteps, StepSize, NumOfNewtonSteps, seed=seed,
                                          chain_offset=start, theta0=th)
                acc, steps, secs = st["accepted"], st["leapfrog_steps"], st["seconds"]
                summ = _t.cat([st["mean"], st["var"], nanmin_rows(st["ess"])], dim=1)
                smp = None
    else:
        smp = _t.zeros((0, S, D), dtype=_t.float64, device=odev)
        acc = _t.zeros(0, dtype=_t.int64, device=odev); steps = _t.zeros(0, dtype=_t.int64, device=odev); secs = 0.0
        summ = _t.zeros((0, 2 * D + 1), dtype=_t.float64, device=odev)
    # timing: the job is as slow as its slowest rank
    tt = _t.tensor([secs], dtype=_t.float64, device=cdev)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    seconds = float(tt.item())
    # the ONE exchange of the sharded path: counters and payload gathered to rank 0 from where the sampler left them
    cnt_all = _gather_rows(_t.stack([acc, steps], dim=1).to(cdev), counts)
    payload = _gather_rows((smp if gather == "samples" else summ).to(cdev), counts)
    if rank != 0:
        return None
    cnt_all = cnt_all.cpu().numpy()
    if gather == "samples":
        payload = payload.cpu().numpy()   # the drop-in contract returns host arrays; the transfer happens once, on rank 0
    else:
        g = payload.cpu().numpy()
        payload = dict(mean=g[:, :D], var=g[:, D:2 * D], min_ess=g[:, 2 * D])
    info = dict(accepted=cnt_all[:, 0], leapfrog_steps=cnt_all[:, 1], world=world, counts=counts)
    return payload, seconds, info


def _sharded_to(sampler, args, XX, t, n_chains, n_iter, burn_in, seed, theta0, alpha, gather, lib, options, gpu, odev, cdev, start, end,
                counts, diagnostics=False, max_lag=None, compat=False, quantiles=None):
    """sample_sharded for the samplers that run through include/rmhmc_out.h: same shards, same gathers, the sampler's own counters;
    diagnostics: one more gather, of every rank's partial (include/rmhmc_diag.h); quantiles: eight all_reduces of every rank's histogram
    (include/rmhmc_quant.h), while the shard's samples and its context are there.  compat: RMHMC's guards (shard_flags)"""
    import torch as _t
    dist = _dist()
    rank, world = dist.get_rank(), dist.get_world_size()
    key = _SHARDED[sampler][0]
    N, D = XX.shape
    n_local, S = end - start, n_iter - burn_in
    counters = _capi.SAMPLERS_TO[key][1]
    if n_local > 0:
        if theta0 is not None:
            args["theta0"] = np.broadcast_to(theta0, (n_chains, D))[start:end]
        with lib.context(N, D, n_local, flags=shard_flags(sampler, D, n_chains, N, compat), device=gpu, options=options) as ctx:
            ctx.set_data(XX, t, alpha)
            st = ctx.sample_to(key, n_iter, burn_in, where="device", device=odev, samples=gather == "samples" or quantiles is not None,
                               stats=gather == "summary", seed=seed, chain_offset=start, diagnostics=diagnostics, max_lag=max_lag, **args)
            qt = _sharded_quantiles(ctx, st["samples"], quantiles, D, cdev, lib) if quantiles is not None else None
        part = st["diag_partial"] if diagnostics else None
        secs = st["seconds"]
        payload = st["samples"] if gather == "samples" else _t.cat([st["mean"], st["var"], nanmin_rows(st["ess"])], dim=1)
        cnt = {k: st[k] for k, _ in counters}
    else:
        secs = 0.0
        payload = _t.zeros((0, S, D) if gather == "samples" else (0, 2 * D + 1), dtype=_t.float64, device=odev)
        cnt = {k: _t.zeros((0, D) if vec else (0,), dtype=_t.float64 if vec else _t.int64, device=odev) for k, vec in counters}
        part = _t.from_numpy(_capi.diag_identity(_capi.diag_lags(S, max_lag)[1], D)).to(odev) if diagnostics else None
        qt = _sharded_quantiles(None, None, quantiles, D, cdev, lib) if quantiles is not None else None
    tt = _t.tensor([secs], dtype=_t.float64, device=cdev)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    ints = [k for k, vec in counters if not vec]
    cnt_all = _gather_rows(_t.stack([cnt[k] for k in ints], dim=1).to(cdev), counts)
    vecs = {k: _gather_rows(cnt[k].to(cdev), counts) for k, vec in counters if vec}   # (AMH's final ProposalSD)
    payload = _gather_rows(payload.to(cdev), counts)
    parts = _gather_rows(part[None].to(cdev), [1] * world) if diagnostics else None   # [world][4 + T][D], in rank order
    if rank != 0:
        return None
    cnt_all = cnt_all.cpu().numpy()
    g = payload.cpu().numpy()
    if gather == "summary":
        g = dict(mean=g[:, :D], var=g[:, D:2 * D], min_ess=g[:, 2 * D])
    info = {k: cnt_all[:, i] for i, k in enumerate(ints)}
    info.update({k: v.cpu().numpy() for k, v in vecs.items()})
    info.update(world=world, counts=counts)
    if diagnostics:
        dg = _capi.diag_finish(list(parts.cpu().numpy()), S // 2, lib=lib)
        info.update({k: dg[k] for k in _capi.DIAG_KEYS})
    if quantiles is not None:
        info.update(quantiles=qt["quantiles"], quantile_draws=qt["draws_used"])
    return g, float(tt.item()), info


def _sharded_quantiles(ctx, samples, probs, D, cdev, lib):
    """The select of include/rmhmc_quant.h over the shards: per round this rank's histogram (ctx None: an empty shard, the identity without
    a launch) is summed over the ranks by one all_reduce where the collective runs, and every rank steps on the sum"""
    import torch as _t
    dist = _dist()

    def hist(round, prefix, K):
        h = ctx.quant_hist(samples, round, prefix) if ctx is not None else _t.from_numpy(_capi.quant_identity(K, D))
        h = h.to(cdev)
        dist.all_reduce(h, op=dist.ReduceOp.SUM)
        return [h]
    return _capi.quant_select(hist, probs, D, lib=lib)
