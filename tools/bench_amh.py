#!/usr/bin/env python3
"""Adaptive Metropolis (include/rmhmc_amh.h) on the MI355X: one JSON line per measurement.

  australian   the reference's own run (main.py data, 1 chain, 10 000 iterations, BurnIn 5 000): TimeTaken, proposals/s, min-ESS/s
  batch        8192 chains x D 64 x M 10 000 synthetic, 5 warm-up sweeps (iterations 0-4, burn-in) then 20 timed sweeps: proposals/s
               and the fraction of the fp64 VALU peak from the stated operation count (AMH_VALU_PER_ROW of csrc/amh.hip.h per data row
               and proposal - an ESTIMATE of the ocml exp / log sequences, not counted from the ISA; peak 78.6 TFLOP/s = 39.3e12 fp64
               lane-instructions/s, counting an FMA as one)
The reference's CPU figure is not measured here: it is the quoted number the comparison is made against (4.7 s for the 5 000
post-burn-in iterations of its NumPy AMH on the same data), labelled as such in the output.

    python tools/bench_amh.py [--only australian|batch] [--chains N]
"""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from riemannhamiltonianmontecarlo_amd import AMH, _capi, tools  # noqa: E402
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg  # noqa: E402

FP64_VALU_LANE_OPS = 78.6e12 / 2


def valu_per_row():
    src = open(os.path.join(ROOT, "riemannhamiltonianmontecarlo_amd", "csrc", "amh.hip.h")).read()
    return int(re.search(r"#define AMH_VALU_PER_ROW (\d+)", src).group(1))


def australian():
    d = np.load(os.path.join(ROOT, "tests", "golden", "data_australian.npz"))
    XX, t = d["XX"], d["t"]
    N, B = 10000, 5000
    w, secs, info = AMH(XX, t, NumOfIterations=N, BurnIn=B, seed=2024, verbose=False, return_info=True)
    ess = tools.CalculateESS(w, w.shape[0] - 1)
    D = XX.shape[1]
    timed = (N - B - 1) * D  # proposals after iteration BurnIn
    return dict(case="amh_australian_1chain", iterations=N, burn_in=B, TimeTaken=secs, proposals_per_s=timed / secs,
                min_ess=float(np.min(ess)), min_ess_per_s=float(np.min(ess)) / secs, acceptance=float(info["acceptance"][0]),
                reference_cpu_TimeTaken_s_quoted_not_measured=4.7)


def batch(n_chains):
    M, D, warm, sweeps = 10000, 64, 5, 20
    XX, t = synthetic_logreg(M, D, 17)
    lib = _capi.load_hip_library()
    with lib.context(M, D, n_chains, flags=0) as ctx:
        ctx.set_data(XX, t)
        # burn_in = warm - 1: iterations 0..warm-1 run before the timer, warm..warm+sweeps-1 are timed
        smp, acc, sd, secs = ctx.amh_sample(warm + sweeps, warm - 1, seed=5)
    props = float(n_chains) * D * sweeps
    ops = props * M * valu_per_row()
    return dict(case="amh_batch", chains=n_chains, D=D, M=M, warmup_sweeps=warm, timed_sweeps=sweeps, seconds=secs,
                proposals_per_s=props / secs, valu_ops_per_row_estimate=valu_per_row(),
                valu_fraction_of_fp64_peak_from_estimate=ops / secs / FP64_VALU_LANE_OPS,
                acceptance=float(acc.sum()) / (float(n_chains) * D * (warm + sweeps)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("australian", "batch"))
    ap.add_argument("--chains", type=int, default=8192)
    a = ap.parse_args()
    if a.only in (None, "australian"):
        print(json.dumps(australian()), flush=True)
    if a.only in (None, "batch"):
        print(json.dumps(batch(a.chains)), flush=True)


if __name__ == "__main__":
    main()
