#!/usr/bin/env python3
"""Posterior quantiles (include/rmhmc_quant.h), first measurements: Context.quantiles on draws that are already in device memory, next
to the same quantiles from torch.sort on the same tensor - what a user would otherwise write, a yardstick outside the library.  One
process per case, ONE run of each in it, one JSON line appended to profiles/quant_bench.jsonl:

  quantiles_call_seconds (host wall time of the second call of the process for the five probabilities 0.025, 0.25, 0.5, 0.75, 0.975:
  eight rounds, each a launch, a copy of the histogram to the host and a step there; the first, untimed call loads the code objects),
  round_kernel_seconds / round_bytes_per_second (per round the library's event timer around k_quant_hist, key "quant_hist", in a
  composition of the pieces of its own; a round reads the tensor once, so bytes = 8 N P), torch_sort_seconds (host wall time between two
  device synchronises of: sort of the [N][P] view along the draws, the ten order statistics gathered, the same interpolation; after an
  untimed sort of a slice), torch_sort_peak_bytes (peak allocated above the tensor itself) and whether the two results are the same
  bits.

config3shape: 8192 chains x 500 draws x D 64 of N(0, 1 / D) entries (their values do not change what either side does, apart from
which bins fill).  australian8192: the draws of 8192 AMH chains on the australian data (1000 iterations, the last 500 kept), D 15.

    python tools/bench_quant.py --case config3shape|australian8192 [--chains 8192] [--draws 500] [--out FILE]

Each run is meant to have a time limit of its own, e.g.
    for c in config3shape australian8192; do timeout -k 10 300 python tools/bench_quant.py --case $c || break; done
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from riemannhamiltonianmontecarlo_amd import _capi  # noqa: E402

CASES = ("config3shape", "australian8192")
PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)


def draws_of(case, n, S, lib, dev):
    if case == "config3shape":
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)
        return torch.randn((n, S, 64), dtype=torch.float64, device=dev, generator=gen) / 8.0
    d = np.load(os.path.join(ROOT, "tests", "golden", "data_australian.npz"))
    XX, t = d["XX"], d["t"]
    with lib.context(XX.shape[0], XX.shape[1], n) as ctx:
        ctx.set_data(XX, t)
        return ctx.sample_to("amh", 2 * S, S, where="device", device=dev, samples=True, seed=0)["samples"]


def torch_quantiles(w2, rank, frac):
    """the same quantiles by a full sort: w2 [N][P] (all finite), rank [2Q][P], frac [Q][P] of the plan"""
    s = w2.sort(dim=0).values
    o = s.gather(0, rank) + 0.0
    lo, hi = o[0::2], o[1::2]
    return torch.where(frac == 0.0, lo, torch.addcmul(lo, frac, hi - lo)), o


def measure(case, n, S):
    dev = torch.device("cuda", 0)
    lib = _capi.load_hip_library()
    w = draws_of(case, n, S, lib, dev)
    n, S, P = w.shape
    N = n * S
    out = dict(case=case, chains=n, draws_per_chain=S, N=N, D=int(P), probs=list(PROBS), first_measurement=True, runs=1,
               tensor_bytes=8 * N * P)
    with lib.context(10, 2, 1) as ctx:           # (the calls use the context for its device and stream only)
        ctx.quantiles(w[:64], PROBS)             # untimed: the first launches load the code objects
        t0 = time.perf_counter()
        q = ctx.quantiles(w, PROBS)
        out["quantiles_call_seconds"] = time.perf_counter() - t0
        ctx.kernel_time("enable")                # (calls of their own: the event timers are kept out of the wall time above)
        secs = []

        def hist(r, prefix, K):
            ctx.kernel_time("reset")
            h = ctx.quant_hist(w, r, prefix)
            secs.append(ctx.kernel_time("quant_hist")[0])
            return [h]
        comp = _capi.quant_select(hist, PROBS, P, lib=lib)
        ctx.kernel_time("disable")
    out.update(round_kernel_seconds=secs, round_bytes_per_second=[8.0 * N * P / s if s > 0 else None for s in secs],
               composition_bit_equal=bool(np.array_equal(comp["quantiles"], q["quantiles"])),
               all_finite=bool((q["draws_used"] == N).all()))
    if out["all_finite"]:
        rank, frac = _capi.quant_plan(q["draws_used"], PROBS, lib=lib)
        rank_d, frac_d = torch.from_numpy(rank).to(dev), torch.from_numpy(frac).to(dev)
        w2 = w.reshape(N, P)
        torch_quantiles(w2[:4096], rank_d.clamp(max=4095), frac_d)      # untimed: the sort and element-wise kernels load
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        t0 = time.perf_counter()
        tq, order = torch_quantiles(w2, rank_d, frac_d)
        torch.cuda.synchronize()
        out.update(torch_sort_seconds=time.perf_counter() - t0, torch_sort_peak_bytes=int(torch.cuda.max_memory_allocated(dev) - base))
        # torch.addcmul may or may not fuse the multiply and the add: compare the order statistics to the bit, the quantiles to 1 ulp
        from_sort = _capi.quant_finish(_key(order.cpu().numpy()), frac, q["draws_used"], lib=lib)
        out["order_statistics_bit_equal"] = bool(np.array_equal(from_sort, q["quantiles"]))
        out["max_ulp_to_torch_interpolation"] = float((np.abs(tq.cpu().numpy() - q["quantiles"]) / np.spacing(np.abs(q["quantiles"]))).max())
        out["sort_over_quantiles"] = out["torch_sort_seconds"] / out["quantiles_call_seconds"]
    return out


def _key(x):
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES, required=True)
    ap.add_argument("--chains", type=int, default=8192)
    ap.add_argument("--draws", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quant_bench.jsonl"))
    a = ap.parse_args()
    line = json.dumps(measure(a.case, a.chains, a.draws))
    print(line, flush=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
