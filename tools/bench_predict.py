#!/usr/bin/env python3
"""Posterior predictive probabilities (include/rmhmc_pred.h), first measurements: rmhmc_pred_partial_dev on draws that are already in
device memory, next to the same reduction written with torch on the same device - what a user would otherwise write, a yardstick
outside the library.  One process per case and number of rows, one run of each in it, one JSON line appended to
profiles/predict_bench.jsonl:

  pred_call_seconds (host wall time of the second call of the process, which allocates its scratch, uploads xnew and ends in a device
  synchronise; the first, untimed call on 64 rows loads the code objects), pred_device_seconds (a third call under the library's event
  timers around its three kernels, key "pred"), torch_seconds (host wall time between two device synchronises of: a validity mask,
  then per chunk of rows sigmoid(samples @ Xnew.T) and its three masked column sums; chunks sized to 1 GiB of logits; after an
  untimed chunk), and the largest difference between the two results.

The draws are synthetic: N(0, 1 / D) entries, so the logits are of order one, as a posterior's are; their values do not change what
either side computes.  config3shape: D 64, rows N(0, 1).  australian: D 15, rows drawn with replacement from the data set.

    python tools/bench_predict.py --case config3shape|australian --rows R [--chains 8192] [--draws 500] [--out FILE]

Each run is meant to have a time limit of its own, e.g.
    for R in 1000 10000; do timeout -k 10 300 python tools/bench_predict.py --case australian --rows $R || break; done
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

CASES = ("config3shape", "australian")


def rows_of(case, R, rs):
    if case == "australian":
        XX = np.load(os.path.join(ROOT, "tests", "golden", "data_australian.npz"))["XX"]
        return np.ascontiguousarray(XX[rs.randint(0, XX.shape[0], R)])
    return rs.randn(R, 64)


def torch_reduction(w2, x, t, chunk):
    """[4, R] by torch: m, sum p, sum p^2, sum q over the draws without a non-finite entry"""
    ok = torch.isfinite(w2).all(dim=1)
    okc = ok.to(w2.dtype)[:, None]
    R = x.shape[0]
    out = torch.zeros((4, R), dtype=w2.dtype, device=w2.device)
    out[0] = ok.sum()
    wz = torch.where(ok[:, None], w2, torch.zeros((), dtype=w2.dtype, device=w2.device))
    for a in range(0, R, chunk):
        p = torch.sigmoid(wz @ x[a:a + chunk].T)
        out[1, a:a + chunk] = (p * okc).sum(dim=0)
        out[2, a:a + chunk] = (p * p * okc).sum(dim=0)
        q = torch.where(t[None, a:a + chunk] == 1.0, p, 1.0 - p)
        out[3, a:a + chunk] = (q * okc).sum(dim=0)
    return out


def measure(case, R, n, S):
    rs = np.random.RandomState(0)
    x = rows_of(case, R, rs)
    D = x.shape[1]
    t = (rs.rand(R) < 0.5).astype(np.float64)
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    w = torch.randn((n, S, D), dtype=torch.float64, device=dev, generator=gen) / np.sqrt(D)
    N = n * S
    out = dict(case=case, chains=n, draws_per_chain=S, N=N, D=int(D), R=R, first_measurement=True, runs=1)
    lib = _capi.load_hip_library()
    with lib.context(10, 2, 1) as ctx:           # (the call uses the context for its device and stream only)
        ctx.predict_partial(w, x[:64], t[:64])   # untimed: the first launches load the code objects
        t0 = time.perf_counter()
        part = ctx.predict_partial(w, x, t)
        out["pred_call_seconds"] = time.perf_counter() - t0
        ctx.kernel_time("enable")                # (a call of its own: the event timers are kept out of the wall time above)
        ctx.kernel_time("reset")
        again = ctx.predict_partial(w, x, t)
        s, k = ctx.kernel_time("pred")
        ctx.kernel_time("disable")
        out.update(pred_device_seconds=s, pred_launch_groups=k, repeat_bit_equal=bool(torch.equal(part, again)))
    chunk = max(1, (1 << 30) // (8 * N))
    xd, td = torch.from_numpy(x).to(dev), torch.from_numpy(t).to(dev)
    w2 = w.reshape(N, D)
    torch_reduction(w2[:4096], xd[:chunk], td[:chunk], chunk)      # untimed: rocBLAS and the element-wise kernels load
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ref = torch_reduction(w2, xd, td, chunk)
    torch.cuda.synchronize()
    out.update(torch_seconds=time.perf_counter() - t0, torch_chunk_rows=chunk)
    out["max_abs_diff_of_means"] = float(((part[1:] - ref[1:]).abs() / N).max())
    out["draws_used_equal"] = bool((part[0] == ref[0]).all())
    out["flops_product"] = 2.0 * R * N * D
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES, required=True)
    ap.add_argument("--rows", type=int, required=True)
    ap.add_argument("--chains", type=int, default=8192)
    ap.add_argument("--draws", type=int, default=500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predict_bench.jsonl"))
    a = ap.parse_args()
    line = json.dumps(measure(a.case, a.rows, a.chains, a.draws))
    print(line, flush=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
