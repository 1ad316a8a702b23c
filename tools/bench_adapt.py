#!/usr/bin/env python3
"""The warm-up of fixed-metric HMC against the hand-set tuning, first measurements: PHMC from the identity mass with warmup=500 (step
size by dual averaging, mass from the pooled covariance of all chains, include/rmhmc_adapt.h) and PHMC with mass = the metric at the
posterior mode at eps = 0.5 (today's defaults).  One process per data set, one run of each arm in it, one JSON line per arm appended
to profiles/adapt_bench.jsonl:

  warm-up seconds (arm "warmup") or the seconds of the mode search (arm "mode"), the step size and the acceptance of the sampling
  run, TimeTaken (the sampler's own timer), the mean per-chain min-ESS and min-ESS/s per chain, the maximum split R-hat, and for the
  warm-up its traces and the device time of the covariance kernels per window (rmhmc_kernel_time "cov", from a second, short warm-up
  with the library's event timers on: they replace the graph replay, so it is kept out of the timed run).

    python tools/bench_adapt.py --case australian8192|config3 [--iters N --burn-in B --warmup U] [--only warmup|mode]

Each case is meant to run under a time limit of its own, e.g.
    timeout -k 10 600 python tools/bench_adapt.py --case australian8192 && timeout -k 10 900 python tools/bench_adapt.py --case config3
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from riemannhamiltonianmontecarlo_amd import _capi  # noqa: E402
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg  # noqa: E402

CASES = {"australian8192": ("australian", 8192), "config3": ("syn_m10000_d64", 8192)}


def load(case):
    name, n = CASES[case]
    if name == "australian":
        d = np.load(os.path.join(ROOT, "tests", "golden", "data_australian.npz"))
        return d["XX"], d["t"], n
    XX, t = synthetic_logreg(10000, 64, 0)   # bench.py's generator for config 3
    return XX, t, n


def measure(case, arm, n_iter, burn_in, warmup, window):
    import torch
    XX, t, n = load(case)
    N, D = XX.shape
    lib = _capi.load_hip_library()
    dev = torch.device("cuda", 0)
    out = dict(case=case, arm=arm, chains=n, M=int(N), D=int(D), iterations=n_iter, burn_in=burn_in, L=6, first_measurement=True)
    with lib.context(N, D, n, flags=0) as ctx:
        ctx.set_data(XX, t)
        kw = dict(where="device", device=dev, samples=True, stats=True, seed=2024)
        if arm == "warmup":
            length, kind = _capi.adapt_schedule(warmup, window)
            ctx.phmc_set_mass(None)
            w = ctx.phmc_warmup(length, kind, L=6, eps0=0.5, seed=2024)
            eps, theta0 = w["step_size"], w["theta"]
            out.update(warmup=warmup, window=window, min_rows=10 * int(D), warmup_seconds=w["seconds"], eps_trace=w["eps_trace"].tolist(),
                       accept_trace=w["accept_trace"].tolist(), mass_updated=w["mass_updated"].tolist())
        else:
            t0 = time.perf_counter()
            m = ctx.phmc_mode()
            out.update(newton_iters=m["iters"], newton_seconds=time.perf_counter() - t0, newton_converged=m["converged"])
            ctx.phmc_set_mass(m["G"])
            eps, theta0 = 0.5, m["w"]
        r = ctx.phmc_sample_to(n_iter, burn_in, L=6, eps=eps, theta0=theta0, **kw)
        secs = r["seconds"]
        mine = r["ess"].cpu().numpy().min(axis=1)
        dg = ctx.diagnose(r["samples"])
        out.update(step_size=eps, TimeTaken=secs, acceptance=float(r["accepted"].sum().item()) / (n * n_iter),
                   min_ess_per_chain_mean=float(np.nanmean(mine)), min_ess_per_s_per_chain=float(np.nanmean(mine) / secs),
                   chains_with_ess=int(np.isfinite(mine).sum()), rhat_max=float(np.nanmax(dg["rhat"])),
                   ess_pooled_min=float(np.nanmin(dg["ess_pooled"])))
        if arm == "warmup":   # the covariance kernels' device time, from a short warm-up under the event timers
            del r
            ctx.kernel_time("enable")
            ctx.kernel_time("reset")
            ctx.phmc_set_mass(None)
            ctx.phmc_warmup([window] * 4, [0, 1, 1, 0], L=6, eps0=0.5, seed=1)
            cs, ck = ctx.kernel_time("cov")
            ctx.kernel_time("disable")
            out.update(cov_kernels_us_per_window=1e6 * cs / max(ck, 1), cov_windows_timed=int(ck), cov_rows_per_window=int(n * window))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=tuple(CASES), required=True)
    ap.add_argument("--only", choices=("warmup", "mode"))
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--burn-in", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--window", type=int, default=25)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adapt_bench.jsonl"))
    a = ap.parse_args()
    for arm in ([a.only] if a.only else ["warmup", "mode"]):
        line = json.dumps(measure(a.case, arm, a.iters, a.burn_in, a.warmup, a.window))
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
