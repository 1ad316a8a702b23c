#!/usr/bin/env python3
"""Auxiliary-variable Gibbs sampler (include/rmhmc_gibbs.h) on the MI355X: one JSON line per measurement.

  australian   the reference's own run (main.py data, 1 chain, max_iter 10 000, burn_in 5 000): time, iterations/s, min-ESS/s, capped
               rows, and the posterior mean / sd of every coefficient
  batch        8192 chains x D 64 x M 10 000 synthetic: a few iterations before the timer (burn-in), then --timed timed ones:
               iterations/s, row updates/s (chains x M x iterations / s), ms per iteration; with --kernels the per-kernel event times of
               the library (rmhmc_kernel_time) for the split between assembly, factor, B, sweep, beta and mixing-weight kernels
The reference's CPU figure is quoted, not measured alongside: about 0.5 s per iteration of its gibbs_sampler.py on australian (0.35 s
on pima) on one CPU core, i.e. about 2 500 s for the 5 000 timed iterations.

    python tools/bench_gibbs.py [--only australian|batch] [--chains N] [--timed K] [--warm W] [--kernels]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from riemannhamiltonianmontecarlo_amd import _capi, auxiliary_gibbs, tools  # noqa: E402
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg  # noqa: E402

KERNELS = ("gibbs_assemble", "gibbs_factor", "gibbs_b", "gibbs_sweep", "gibbs_beta", "gibbs_mix")


def australian():
    d = np.load(os.path.join(ROOT, "tests", "golden", "data_australian.npz"))
    XX, t = d["XX"], d["t"]
    N, B = 10000, 5000
    w, secs, info = auxiliary_gibbs(XX, t, max_iter=N, burn_in=B, seed=2024, verbose=False, return_info=True)
    ess = tools.CalculateESS(w, w.shape[0] - 1)
    return dict(case="gibbs_australian_1chain", iterations=N, burn_in=B, time=secs, iterations_per_s=(N - B) / secs,
                min_ess=float(np.min(ess)), min_ess_per_s=float(np.min(ess)) / secs, capped=int(info["capped"].sum()),
                stopped=int(info["stopped"][0]),
                all_finite=bool(np.isfinite(w).all()), posterior_mean=[float(x) for x in w.mean(axis=0)],
                posterior_sd=[float(x) for x in w.std(axis=0)], reference_cpu_s_per_iteration_quoted_not_measured=0.5)


def batch(n_chains, timed, warm, kernels):
    M, D = 10000, 64
    XX, t = synthetic_logreg(M, D, 17)
    lib = _capi.load_hip_library()
    with lib.context(M, D, n_chains, flags=0) as ctx:
        ctx.set_data(XX, t)
        if kernels:
            ctx.kernel_time("enable")
        # burn_in = warm: iterations 0..warm-1 run before the timer, warm..warm+timed-1 are timed
        r = ctx.gibbs_sample(warm + timed, warm, seed=5)
        smp, capped, secs, alive = r["samples"], r["capped"], r["seconds"], r["stopped"] < 0
        split = {k: ctx.kernel_time(k)[0] / (warm + timed) * 1e3 for k in KERNELS} if kernels else None
    per_iter = secs / timed
    out = dict(case="gibbs_batch", chains=n_chains, D=D, M=M, warmup_iterations=warm, timed_iterations=timed, seconds=secs,
               ms_per_iteration=per_iter * 1e3, iterations_per_s=timed / secs, chain_iterations_per_s=n_chains * timed / secs,
               row_updates_per_s=n_chains * M * timed / secs, capped=int(capped[alive].sum()), chains_stopped_on_lam_inf=int((~alive).sum()),
               all_finite=bool(np.isfinite(smp[alive]).all()))
    if split:
        out["kernel_ms_per_iteration"] = split
        out["sweep_ns_per_row_per_chain"] = split["gibbs_sweep"] * 1e6 / (n_chains * M)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("australian", "batch"))
    ap.add_argument("--chains", type=int, default=8192)
    ap.add_argument("--timed", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    if a.only in (None, "australian"):
        print(json.dumps(australian()), flush=True)
    if a.only in (None, "batch"):
        print(json.dumps(batch(a.chains, a.timed, a.warm, a.kernels)), flush=True)


if __name__ == "__main__":
    main()
