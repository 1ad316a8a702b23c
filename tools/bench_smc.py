#!/usr/bin/env python3
"""Adaptive sequential Monte Carlo (include/rmhmc_smc.h), first measurements: the log marginal likelihood of one data set with 8192
particles, PHMC's defaults (L 6, eps 0.5), cess_target 0.9, resample_below 0.5, one transition per stage and a mass update in every
stage, four seeds 20 001 apart (a run of seed s draws from the streams of s .. s + its number of stages: neighbouring seeds would share
random numbers).  One process per case, one JSON line appended to profiles/smc_bench.jsonl:

  per seed the stages taken, the seconds (host wall time of rmhmc_smc_run, which ends in a device synchronise; after an untimed run of
  at most 16 stages), log Z, the mean acceptance and the stages that resampled; the spread of log Z over the seeds (standard deviation,
  and the log of the mean estimate with its delta-method standard error); the Laplace value; beside them the rows of
  profiles/ais_bench.jsonl for the case (rmhmc_ais_run on the power4 ladder, as measured when it was added), and a fresh rmhmc_ais_run at
  the number of stages the first seed took (same process, same context), for the per-stage overhead of the adaptive run:
  overhead_us_per_stage = seconds / stages of the adaptive run - seconds / stages of that run.

    python tools/bench_smc.py --case australian|config3 [--chains N] [--seeds K] [--out FILE]

Each run is meant to have a time limit of its own, e.g.
    for c in australian config3; do timeout -k 10 600 python tools/bench_smc.py --case $c || break; done
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
from riemannhamiltonianmontecarlo_amd.evidence import log_laplace  # noqa: E402

CASES = ("australian", "config3")


def load(case):
    if case == "australian":
        d = np.load(os.path.join(ROOT, "tests", "golden", "data_australian.npz"))
        return d["XX"], d["t"]
    return synthetic_logreg(10000, 64, 0)   # bench.py's generator for config 3


def ais_rows(case):
    path = os.path.join(ROOT, "profiles", "ais_bench.jsonl")
    keep = ("stages", "seconds", "log_evidence", "se", "weight_ess")
    return [{k: r[k] for k in keep} for r in map(json.loads, open(path)) if r["case"] == case] if os.path.exists(path) else []


def measure(case, n, seeds, rho, tau):
    XX, t = load(case)
    N, D = XX.shape
    lib = _capi.load_hip_library()
    out = dict(case=case, chains=n, M=int(N), D=int(D), cess_target=rho, resample_below=tau, L=6, eps=0.5, mass_every=1, stage_len=1,
               first_measurement=True, runs_per_seed=1)
    with lib.context(N, D, n, flags=0) as ctx:
        ctx.set_data(XX, t)
        t0 = time.perf_counter()
        md = ctx.phmc_mode()
        out.update(newton_iters=md["iters"], newton_seconds=time.perf_counter() - t0, newton_converged=md["converged"])
        H = md["G"] - np.eye(D) / 100.0
        ctx.phmc_set_mass(None)
        ctx.smc_run(rho, tau, 16, 1, 1, H, L=6, eps=0.5, seed=7)        # untimed: the first launches load the code objects
        runs = []
        for s in range(seeds):
            ctx.phmc_set_mass(None)
            r = ctx.smc_run(rho, tau, 20000, 1, 1, H, L=6, eps=0.5, seed=2024 + 20001 * s)
            runs.append(dict(seed=2024 + 20001 * s, stages=r["T"], seconds=r["seconds"], log_z=r["log_z"], se=r["se"], reached_one=bool(r["beta"][-1] == 1.0),
                             accept_mean=float(r["accept_trace"].mean()), accept_min=float(r["accept_trace"].min()),
                             resampled=int(((r["flags"] & _capi.SMC_RESAMPLED) > 0).sum()), floored=int(((r["flags"] & _capi.SMC_FLOOR) > 0).sum()),
                             cess_min=float(r["cess"].min()), ess_min=float(r["ess"].min()), final_weight_ess=r["weight_ess"],
                             first_beta=float(r["beta"][0])))
        lz = np.array([r["log_z"] for r in runs])
        z = np.exp(lz - lz.max())
        out.update(seeds=runs, log_z_mean=float(lz.mean()), log_z_sd=float(lz.std(ddof=1)) if seeds > 1 else None,
                   log_mean_z=float(lz.max() + np.log(z.mean())), log_mean_z_se=float(z.std(ddof=1) / np.sqrt(seeds) / z.mean()) if seeds > 1 else None,
                   log_laplace=log_laplace(XX, t, md["w"], md["G"]), ais_rows=ais_rows(case))
        T = runs[0]["stages"]
        ctx.phmc_set_mass(None)
        a = ctx.ais_run(*_capi.ais_schedule(T, "power4", 1), H, L=6, eps=0.5, seed=2024)
        out["ais_same_stages"] = dict(stages=T, seconds=a["seconds"], log_evidence=a["log_mean_w"], se=a["se"], weight_ess=a["weight_ess"])
        out["smc_us_per_stage"] = 1e6 * runs[0]["seconds"] / T
        out["ais_us_per_stage"] = 1e6 * a["seconds"] / T
        out["overhead_us_per_stage"] = out["smc_us_per_stage"] - out["ais_us_per_stage"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES, required=True)
    ap.add_argument("--chains", type=int, default=8192)
    ap.add_argument("--seeds", type=int, default=4)
    ap.add_argument("--cess-target", type=float, default=0.9)
    ap.add_argument("--resample-below", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smc_bench.jsonl"))
    a = ap.parse_args()
    line = json.dumps(measure(a.case, a.chains, a.seeds, a.cess_target, a.resample_below))
    print(line, flush=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
