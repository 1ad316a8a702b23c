#!/usr/bin/env python3
"""min-ESS/s of the three Hamiltonian samplers side by side, first measurements: fixed-metric HMC (PHMC, mass = the metric at the
posterior mode, L 6, eps 0.5), plain HMC (L 100, eps 0.14) and RMHMC (L 6, eps 0.5, K 4, the int8 auto rule where it applies).
One process per data set, one run of each sampler in it, one JSON line per sampler appended to profiles/phmc_bench.jsonl:

  TimeTaken (the sampler's own timer: the transitions after burn-in), leapfrog steps/s, acceptance, the mean per-chain min-ESS and
  min-ESS/s (per chain and for the batch), the maximum split R-hat over the dimensions (two chains or more), and for PHMC the Newton
  iterations and seconds of the mode search.  A second, short PHMC run with the library's event timers on (which replace the graph
  replay, so it is kept out of the timed run) gives the device time of the head and tail kernels beside the gradient pass's.

    python tools/bench_phmc.py --case australian1|australian8192|config3 [--iters N --burn-in B] [--only PHMC|HMC|RMHMC]

Each case is meant to run under a time limit of its own, e.g.
    timeout -k 10 900 python tools/bench_phmc.py --case australian1 && timeout -k 10 900 python tools/bench_phmc.py --case australian8192
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

CASES = {"australian1": ("australian", 1), "australian8192": ("australian", 8192), "config3": ("syn_m10000_d64", 8192)}


def load(case):
    name, n = CASES[case]
    if name == "australian":
        d = np.load(os.path.join(ROOT, "tests", "golden", "data_australian.npz"))
        return d["XX"], d["t"], n
    XX, t = synthetic_logreg(10000, 64, 0)   # bench.py's generator for config 3
    return XX, t, n


def measure(case, sampler, n_iter, burn_in):
    import torch
    XX, t, n = load(case)
    N, D = XX.shape
    lib = _capi.load_hip_library()
    dev = torch.device("cuda", 0)
    flags = _capi.auto_metric_flags(D, n, None, M=N) if sampler == "RMHMC" else 0
    out = dict(case=case, sampler=sampler, chains=n, M=int(N), D=int(D), iterations=n_iter, burn_in=burn_in, first_measurement=True)
    with lib.context(N, D, n, flags=(_capi.COMPAT | flags) if sampler == "RMHMC" else 0) as ctx:   # (the shims' flags)
        ctx.set_data(XX, t)
        kw = dict(where="device", device=dev, samples=True, stats=True, seed=2024)
        if sampler == "PHMC":
            t0 = time.perf_counter()
            m = ctx.phmc_mode()
            out.update(newton_iters=m["iters"], newton_seconds=time.perf_counter() - t0, newton_converged=m["converged"])
            ctx.phmc_set_mass(m["G"])
            L = 6
            r = ctx.phmc_sample_to(n_iter, burn_in, L=6, eps=0.5, theta0=m["w"], **kw)
        elif sampler == "HMC":
            L = 100
            r = ctx.sample_to("hmc", n_iter, burn_in, **kw)
        else:
            L = 6
            r = ctx.sample_to("rmhmc", n_iter, burn_in, **kw)
        secs = r["seconds"]
        ess = r["ess"].cpu().numpy()
        mine = ess.min(axis=1)
        steps = float(r["leapfrog_steps"].sum().item())
        out.update(L=L, TimeTaken=secs, leapfrog_steps_per_s=steps / secs, mean_steps_per_transition=steps / (n * (n_iter - burn_in - 1.0)),
                   acceptance=float(r["accepted"].sum().item()) / (n * n_iter), min_ess_per_chain_mean=float(np.nanmean(mine)),
                   min_ess_per_s_per_chain=float(np.nanmean(mine) / secs), min_ess_per_s_batch=float(np.nansum(mine) / secs),
                   chains_with_ess=int(np.isfinite(mine).sum()), int8_metric=bool(flags))
        if n >= 2:
            dg = ctx.diagnose(r["samples"])
            out.update(rhat_max=float(np.nanmax(dg["rhat"])), ess_pooled_min=float(np.nanmin(dg["ess_pooled"])))
        if sampler == "PHMC":   # the kernels' share, from a short run under the event timers
            del r
            ctx.kernel_time("enable")
            ctx.kernel_time("reset")
            ctx.phmc_sample_to(24, 4, L=6, eps=0.5, theta0=m["w"], samples=True, seed=1)
            ph, kp = ctx.kernel_time("phmc")
            rp, kr = ctx.kernel_time("rowpass")
            ctx.kernel_time("disable")
            out.update(phmc_kernels_us_per_launch=1e6 * ph / max(kp, 1), rowpass_us_per_launch=1e6 * rp / max(kr, 1),
                       phmc_share_of_step=2 * ph / max(kp, 1) / (2 * ph / max(kp, 1) + rp / max(kr, 1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=tuple(CASES), required=True)
    ap.add_argument("--only", choices=("PHMC", "HMC", "RMHMC"))
    ap.add_argument("--iters", type=int, default=6000)
    ap.add_argument("--burn-in", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phmc_bench.jsonl"))
    a = ap.parse_args()
    for s in ([a.only] if a.only else ["PHMC", "HMC", "RMHMC"]):
        line = json.dumps(measure(a.case, s, a.iters, a.burn_in))
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
