#!/usr/bin/env python3
"""Time of the cross-chain diagnostics (include/rmhmc_diag.h) against the per-chain ESS kernel on the same tensor: one JSON line.

  A torch.randn tensor of --chains x --samples x --dims float64 on the GPU (8192 x 500 x 64: 2.1 GB), and three calls on it, each
  warmed up once and then timed --repeats times with a host clock around the call (every one of them returns with the library's
  stream idle): Context.diag_partial with every lag (max_lag = H - 1), Context.diag_partial with max_lag = 31, and Context.ess_dev,
  which does the same kind of work per series (one wavefront per series, every lag pair until the Geyer sum stops).  Reported: the
  median and the minimum of each, the ratios of the medians to ess_dev, and what the all-lag call computes: fp64 FMAs of the lag loop
  as the kernel runs it (the triangle in steps of 16 rows and 16 lags) over the median time.

    python tools/bench_diag.py [--chains N --samples S --dims P] [--repeats R] [--out profiles/diag_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def lag_loop_fmas(n, S, P, T):
    """FMAs k_diag_acov issues for useful columns: per series and dimension, for every group of 16 lags starting at tg < T, the row
    steps s0 = 0, 16, .. < H - tg, 256 FMAs each"""
    H = S // 2
    steps = sum((H - tg + 15) // 16 for tg in range(0, T, 16))
    return 2 * n * P * steps * 256


def timed(fn, repeats):
    import torch
    fn()                                   # warm-up: code objects, the LDS attribute, the allocator
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()                               # (returns with the library's stream idle)
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=8192)
    ap.add_argument("--samples", type=int, default=500)
    ap.add_argument("--dims", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from riemannhamiltonianmontecarlo_amd import _capi
    lib = _capi.load_hip_library()
    n, S, P = a.chains, a.samples, a.dims
    H = S // 2
    torch.manual_seed(0)
    x = torch.randn((n, S, P), dtype=torch.float64, device="cuda:0")
    with lib.context(20, 2, 1) as ctx:
        runs = {"diag_all_lags": timed(lambda: ctx.diag_partial(x, H - 1), a.repeats),
                "diag_max_lag_31": timed(lambda: ctx.diag_partial(x, min(31, H - 1)), a.repeats),
                "ess_dev": timed(lambda: ctx.ess_dev(x), a.repeats)}
        dg = ctx.diagnose(x, H - 1)
    med = {k: statistics.median(v) for k, v in runs.items()}
    fmas = lag_loop_fmas(n, S, P, H)
    rec = {"case": "diag_bench", "chains": n, "samples": S, "dims": P, "H": H, "repeats": a.repeats, "samples_bytes": n * S * P * 8}
    for k, v in runs.items():
        rec[k + "_s_median"] = med[k]
        rec[k + "_s_min"] = min(v)
    rec.update(all_lags_over_ess_dev=med["diag_all_lags"] / med["ess_dev"], max_lag_31_over_ess_dev=med["diag_max_lag_31"] / med["ess_dev"],
               lag_loop_fmas=fmas, lag_loop_tflops_fp64=2 * fmas / med["diag_all_lags"] / 1e12,
               max_lag_31_bytes_per_s=n * S * P * 8 / med["diag_max_lag_31"],
               rhat_max=float(dg["rhat"].max()), ess_pooled_min=float(dg["ess_pooled"].min()), pairs_max=int(dg["pairs"].max()),
               first_measurement=True)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
