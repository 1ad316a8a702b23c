#!/usr/bin/env python3
"""Annealed importance sampling (include/rmhmc_ais.h), first measurements: the log marginal likelihood of one data set with 8192 chains,
PHMC's defaults (L 6, eps 0.5), the ladder beta_k = (k / T)^4, one transition per stage and a mass update in every stage.  One process
per case and number of stages, one run in it, one JSON line appended to profiles/ais_bench.jsonl:

  seconds (host wall time of rmhmc_ais_run, which ends in a device synchronise; after an untimed run of 16 stages), log Z, its standard error, the weight-ESS, the Laplace value, the acceptance over the
  stages, and the device time per stage of the kernels keyed "ais" (k_tphmc_init, k_tphmc_tail, the weight kernels), "phmc" (the head)
  and "rowpass" - from a second, short run of 32 stages with the library's event timers on (they replace the graph replay, so it is kept
  out of the timed run).

    python tools/bench_ais.py --case australian|config3 --temps T [--chains N] [--out FILE]

Each run is meant to have a time limit of its own, e.g.
    for T in 250 1000 4000; do timeout -k 10 600 python tools/bench_ais.py --case australian --temps $T || break; done
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


def measure(case, T, n):
    XX, t = load(case)
    N, D = XX.shape
    lib = _capi.load_hip_library()
    out = dict(case=case, chains=n, M=int(N), D=int(D), stages=T, ladder="power4", L=6, eps=0.5, mass_every=1, first_measurement=True,
               runs=1)
    with lib.context(N, D, n, flags=0) as ctx:
        ctx.set_data(XX, t)
        t0 = time.perf_counter()
        md = ctx.phmc_mode()
        out.update(newton_iters=md["iters"], newton_seconds=time.perf_counter() - t0, newton_converged=md["converged"])
        H = md["G"] - np.eye(D) / 100.0
        ctx.phmc_set_mass(None)
        ctx.ais_run(*_capi.ais_schedule(16, "power4", 1), H, L=6, eps=0.5, seed=7)      # untimed: the first launches load the code objects
        ctx.phmc_set_mass(None)
        r = ctx.ais_run(*_capi.ais_schedule(T, "power4", 1), H, L=6, eps=0.5, seed=2024)
        out.update(seconds=r["seconds"], log_evidence=r["log_mean_w"], se=r["se"], weight_ess=r["weight_ess"], n_nan=r["n_nan"],
                   log_laplace=log_laplace(XX, t, md["w"], md["G"]), accept_min=float(r["accept_trace"].min()),
                   accept_mean=float(r["accept_trace"].mean()), accept_max=float(r["accept_trace"].max()))
        timed = 32
        ctx.kernel_time("enable")
        ctx.kernel_time("reset")
        ctx.phmc_set_mass(None)
        ctx.ais_run(*_capi.ais_schedule(timed, "power4", 1), H, L=6, eps=0.5, seed=1)
        for key in ("ais", "phmc", "rowpass"):
            s, k = ctx.kernel_time(key)
            out["%s_us_per_stage" % key] = 1e6 * s / timed
            out["%s_launches_per_stage" % key] = k / float(timed)
        ctx.kernel_time("disable")
        out["stages_timed"] = timed
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES, required=True)
    ap.add_argument("--temps", type=int, required=True)
    ap.add_argument("--chains", type=int, default=8192)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ais_bench.jsonl"))
    a = ap.parse_args()
    line = json.dumps(measure(a.case, a.temps, a.chains))
    print(line, flush=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
