#!/usr/bin/env python3
"""min-ESS/s of the baseline samplers at batch scale through the output descriptor (include/rmhmc_out.h): one JSON line per sampler.

  AMH, IWLS, Gibbs on the australian data (690 x 15), 8192 chains, the samplers' default 10 000 / 5 000 iterations, ONE run each: the
  samples stay in HBM (4.9 GB), mean / var / ESS per chain and the run-mean chain with its ESS are reduced there.  Reported: TimeTaken
  (the sampler's own timer: the iterations after burn-in), the per-chain min-ESS (mean and median over the chains that finished; a
  stopped Gibbs chain has none), min-ESS/s per chain and summed over the batch, the run-mean chain's min-ESS (main.py:71).
  Beside it, in the same process, the write-out both ways: `device_write_out_s`, the wall time of the call's own write-out (the
  library's figure, rmhmc_kernel_time "write_out": the ESS kernel over all n x D series, k_run_mean, the ESS of the run mean, the
  copies of the statistics and counters, its allocations; `device_ess_s` = rmhmc_ess_dev alone on the same buffer), against
  `host_copy_s` (the samples to host memory) + `host_numpy_ess_s` (tools.CalculateESS chain by chain, measured on the first
  --host-chains chains only and scaled to all of them in `host_numpy_ess_s_scaled`; the host run mean and its ESS are not in it).

    python tools/bench_summary.py [--only AMH|IWLS|Gibbs] [--chains N] [--iters N --burn-in B] [--host-chains K]
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from riemannhamiltonianmontecarlo_amd import _capi, tools  # noqa: E402

KEYS = {"AMH": "amh", "IWLS": "iwls", "Gibbs": "gibbs"}


def measure(name, n_chains, n_iter, burn_in, host_chains):
    import torch
    d = np.load(os.path.join(ROOT, "tests", "golden", "data_australian.npz"))
    XX, t = d["XX"], d["t"]
    N, D = XX.shape
    lib = _capi.load_hip_library()
    dev = torch.device("cuda", 0)
    flags = _capi.auto_metric_flags(D, n_chains, None, M=N) if name == "IWLS" else 0
    with lib.context(N, D, n_chains, flags=flags) as ctx:
        ctx.set_data(XX, t)
        t0 = time.perf_counter()
        with np.errstate(all="ignore"):
            r = ctx.sample_to(KEYS[name], n_iter, burn_in, where="device", device=dev, samples=True, stats=True, run_mean=True, seed=2024)
        wall = time.perf_counter() - t0
        write_out = ctx.kernel_time("write_out")[0]
        smp = r["samples"]
        t0 = time.perf_counter()
        ess2 = ctx.ess_dev(smp)[0]
        torch.cuda.synchronize()
        device_stats = time.perf_counter() - t0
        same = bool(torch.equal(torch.nan_to_num(ess2, nan=-1.0), torch.nan_to_num(r["ess"], nan=-1.0)))
    ess = r["ess"].cpu().numpy()
    run_ess = r["run_ess"].cpu().numpy()
    secs = r["seconds"]
    t0 = time.perf_counter()
    x = smp.cpu().numpy()
    host_copy = time.perf_counter() - t0
    k = min(host_chains, n_chains)
    t0 = time.perf_counter()
    with np.errstate(all="ignore"):
        ref = np.stack([tools.CalculateESS(x[c], x.shape[1] - 1, "matlab").ravel() for c in range(k)])
    host_ess = time.perf_counter() - t0
    ok = np.isfinite(ess).all(axis=1)
    mine = ess[ok].min(axis=1)
    both = ok[:k] & np.isfinite(ref).all(axis=1)
    out = dict(case="summary_australian_batch", sampler=name, chains=n_chains, iterations=n_iter, burn_in=burn_in, M=int(N), D=int(D),
               TimeTaken=secs, call_wall_s=wall, chain_iterations_per_s=n_chains * (n_iter - burn_in) / secs,
               chains_with_ess=int(ok.sum()), min_ess_per_chain_mean=float(mine.mean()), min_ess_per_chain_median=float(np.median(mine)),
               min_ess_per_s_per_chain=float(mine.mean() / secs), min_ess_per_s_batch=float(mine.sum() / secs),
               run_mean_min_ess=float(np.nanmin(run_ess)) if np.isfinite(run_ess).any() else None,
               samples_bytes=int(x.nbytes), device_write_out_s=write_out, device_ess_s=device_stats, device_stats_equal_the_call=same, host_copy_s=host_copy,
               host_numpy_ess_chains=k, host_numpy_ess_s=host_ess, host_numpy_ess_s_scaled=host_ess * n_chains / k,
               device_vs_numpy_ess_max_rel=float(np.abs(ess[:k][both] / ref[both] - 1).max()) if both.any() else None,
               first_measurement=True)
    if name == "Gibbs":
        st = r["stopped"].cpu().numpy()
        nan_rows = np.isnan(x).any(axis=2).sum(axis=1)
        implied = np.where(st >= 0, np.maximum(0, n_iter - 1 - np.maximum(st, burn_in - 1)), 0)   # rows after the stop iteration
        out.update(stopped_chains=int((st >= 0).sum()), chains_with_nan_rows=int((nan_rows > 0).sum()),
                   stopped_in_the_last_iteration=int((st == n_iter - 1).sum()),
                   nan_rows_equal_those_the_stop_implies=bool(np.array_equal(nan_rows, implied)), capped_rows=int(r["capped"].sum().item()))
    else:
        out.update(acceptance=float(r["accepted"].sum().item()) / (n_chains * n_iter * (D if name == "AMH" else 1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=tuple(KEYS))
    ap.add_argument("--chains", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=10000)
    ap.add_argument("--burn-in", type=int, default=5000)
    ap.add_argument("--host-chains", type=int, default=1024)
    a = ap.parse_args()
    alive = threading.Event()

    def heartbeat():   # (a long run prints nothing by itself)
        t0 = time.perf_counter()
        while not alive.wait(60.0):
            print("... %d s" % (time.perf_counter() - t0), file=sys.stderr, flush=True)

    threading.Thread(target=heartbeat, daemon=True).start()
    for name in ([a.only] if a.only else list(KEYS)):
        print(json.dumps(measure(name, a.chains, a.iters, a.burn_in, a.host_chains)), flush=True)
    alive.set()


if __name__ == "__main__":
    main()
