#!/usr/bin/env python3
"""IWLS Metropolis-Hastings (include/rmhmc_iwls.h) on the MI355X: one JSON line per measurement.

  australian   the reference's own run (main.py data, 1 chain, max_iter 10 000, burn_in 5 000), compat and corrected: TimeTaken,
               iterations/s, min-ESS/s, acceptance, saturated fraction, and the posterior mean / sd of every coefficient
  batch        8192 chains x D 64 x M 10 000 synthetic, both modes: 5 iterations before the timer (burn-in), then 20 timed: chain-iterations/s,
               ms per iteration, the metric-assembly path, and that path's operation count of ONE assembly per iteration over the time of
               a whole iteration as a fraction of the path's peak (int8: 2 M NP S(S+1)/2 integer ops per chain, NP = D(D+1)/2, peak
               5.0e15 op/s; fp64: 2 M NP flop per chain, peak 78.6e12 flop/s - a whole-iteration rate, not the assembly kernel's share)
The reference's CPU figure is not measured here: 1.0 s per 100 post-burn-in iterations of its NumPy iwls on australian, measured once on
the build machine over 200 iterations and extrapolated to the 5 000 timed iterations (about 48 s), labelled as such in the output.

    python tools/bench_iwls.py [--only australian|batch] [--chains N] [--timed K]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from riemannhamiltonianmontecarlo_amd import _capi, iwls, tools  # noqa: E402
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg  # noqa: E402

INT8_MFMA_PEAK = 5.0e15   # op/s dense int8 matrix (bench.py)
FP64_MFMA_PEAK = 78.6e12  # flop/s dense fp64 matrix (bench.py)


def australian(compat):
    d = np.load(os.path.join(ROOT, "tests", "golden", "data_australian.npz"))
    XX, t = d["XX"], d["t"]
    N, B = 10000, 5000
    w, secs, info = iwls(XX, t, max_iter=N, burn_in=B, seed=2024, compat=compat, verbose=False, return_info=True)
    ess = tools.CalculateESS(w, w.shape[0] - 1)
    return dict(case="iwls_australian_1chain", compat=compat, iterations=N, burn_in=B, TimeTaken=secs, iterations_per_s=(N - B) / secs,
                min_ess=float(np.min(ess)), min_ess_per_s=float(np.min(ess)) / secs, acceptance=float(info["acceptance"][0]),
                saturated_fraction=float(info["saturated"][0]) / N, posterior_mean=[float(x) for x in w.mean(axis=0)],
                posterior_sd=[float(x) for x in w.std(axis=0)],
                reference_cpu_TimeTaken_s_extrapolated_not_measured=48.0)


def batch(n_chains, compat, timed):
    M, D, warm = 10000, 64, 5
    XX, t = synthetic_logreg(M, D, 17)
    lib = _capi.load_hip_library()
    flags = _capi.auto_metric_flags(D, n_chains, None, M=M)
    with lib.context(M, D, n_chains, flags=flags) as ctx:
        ctx.set_data(XX, t)
        int8 = ctx.int8_certificate()[1] if flags else 0
        # burn_in = warm: iterations 0..warm-1 run before the timer, warm..warm+timed-1 are timed
        smp, acc, sat, secs = ctx.iwls_sample(warm + timed, warm, compat=compat, seed=5)
    NP = D * (D + 1) // 2
    S = 6
    if int8:
        ops, peak, path = 2.0 * n_chains * M * NP * (S * (S + 1) // 2), INT8_MFMA_PEAK, "int8 matrix cores, %d slices" % S
    else:
        ops, peak, path = 2.0 * n_chains * M * NP, FP64_MFMA_PEAK, "fp64 matrix cores"
    per_iter = secs / timed
    return dict(case="iwls_batch", compat=compat, chains=n_chains, D=D, M=M, warmup_iterations=warm, timed_iterations=timed,
                seconds=secs, ms_per_iteration=per_iter * 1e3, chain_iterations_per_s=n_chains * timed / secs, assembly_path=path,
                assembly_ops_per_iteration=ops, assembly_ops_over_iteration_time_frac_of_peak=ops / per_iter / peak,
                acceptance=float(acc.sum()) / (n_chains * (warm + timed)), saturated=int(sat.sum()),
                all_finite=bool(np.isfinite(smp).all()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("australian", "batch"))
    ap.add_argument("--chains", type=int, default=8192)
    ap.add_argument("--timed", type=int, default=20)
    ap.add_argument("--compat", choices=("both", "1", "0"), default="both")
    a = ap.parse_args()
    modes = (True, False) if a.compat == "both" else (a.compat == "1",)
    if a.only in (None, "australian"):
        for c in modes:
            print(json.dumps(australian(c)), flush=True)
    if a.only in (None, "batch"):
        for c in modes:
            print(json.dumps(batch(a.chains, c, a.timed)), flush=True)


if __name__ == "__main__":
    main()
