#!/usr/bin/env python3
"""PSIS-LOO and WAIC (include/rmhmc_loo.h), first measurements: rmhmc_loo_dev on draws that are already in device memory, next to the
same reduction written with torch on the same device - what a user would otherwise write, a yardstick outside the library.  One process
per case, one run of each in it, one JSON line appended to profiles/loo_bench.jsonl:

  loo_call_seconds (host wall time of the second call of the process, which allocates its scratch, uploads the rows and ends in a
  device synchronise; the first, untimed call on 64 rows loads the code objects), device seconds per stage from a third call under
  the library's event timers (loglik: the validity pass and the product; moments; select: the eight histogram rounds; split; fit),
  torch_seconds (host wall time between two device synchronises of, per chunk of rows: logsigmoid(+-samples @ X.T), the sums of the
  moments, torch.sort along the draws and the tail's sum of weights - no Pareto fit; chunks sized to 1 GiB of log-likelihoods; after
  an untimed chunk; over --torch-rows rows, as many as one is willing to wait for), and the largest difference of lppd between the two.

australian: the data set's own 690 rows, D 15, draws by the recipe of psis_loo (mode by Newton, mass = G(mode), fixed-metric HMC on the
device).  config3shape: D 64, rows N(0, 1), synthetic draws N(0, 1 / D), so that the logits are of order one.

    python tools/bench_loo.py --case australian|config3shape [--rows R] [--chains 8192] [--draws 500] [--torch-rows 128] [--out FILE]

Each run is meant to have a time limit of its own, e.g.
    timeout -k 10 300 python tools/bench_loo.py --case australian && timeout -k 10 300 python tools/bench_loo.py --case config3shape --rows 1000
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

CASES = ("australian", "config3shape")
STAGES = (("loglik", "loo_loglik"), ("moments", "loo_moments"), ("select", "quant_hist"), ("split", "loo_split"), ("fit", "loo_fit"))


def torch_reduction(w2, x, t, chunk, tail):
    """lppd [R], p_waic [R] and the unsmoothed tail weight sum [R] by torch, over the draws without a non-finite entry (all, here)"""
    R = x.shape[0]
    N = w2.shape[0]
    lppd = torch.empty(R, dtype=w2.dtype, device=w2.device); pw = torch.empty_like(lppd); ta = torch.empty_like(lppd)
    sign = torch.where(t == 1.0, 1.0, -1.0).to(w2.dtype)
    for a in range(0, R, chunk):
        ll = torch.nn.functional.logsigmoid((w2 @ x[a:a + chunk].T) * sign[None, a:a + chunk])
        lppd[a:a + chunk] = torch.logsumexp(ll, dim=0) - np.log(N)
        pw[a:a + chunk] = ll.var(dim=0, unbiased=True)
        srt, _ = torch.sort(ll, dim=0)
        ta[a:a + chunk] = torch.exp(srt[0][None] - srt[:tail]).sum(dim=0)
    return lppd, pw, ta


def measure(case, R, n, S, torch_rows):
    rs = np.random.RandomState(0)
    dev = torch.device("cuda", 0)
    lib = _capi.load_hip_library()
    out = dict(case=case, chains=n, draws_per_chain=S, N=n * S, first_measurement=True, runs=1)
    if case == "australian":
        d = np.load(os.path.join(ROOT, "tests", "golden", "data_australian.npz"))
        x, t = np.ascontiguousarray(d["XX"], dtype=np.float64), np.ascontiguousarray(d["t"], dtype=np.float64).reshape(-1)
        R = x.shape[0]
        with lib.context(R, x.shape[1], n) as ctx:
            ctx.set_data(x, t, 100.0)
            md = ctx.phmc_mode()
            ctx.phmc_set_mass(md["G"])
            st = ctx.phmc_sample_to(S + 100, 100, L=6, eps=0.5, where="device", device=dev, samples=True, seed=0, theta0=md["w"])
            w = st["samples"]
            out.update(sampling_seconds=st["seconds"], accept=float(st["accepted"].sum().item()) / (n * (S + 100.0)))
    else:
        x = rs.randn(R, 64)
        t = (rs.rand(R) < 0.5).astype(np.float64)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)
        w = torch.randn((n, S, 64), dtype=torch.float64, device=dev, generator=gen) / 8.0
    D = x.shape[1]
    N = n * S
    out.update(D=int(D), R=int(R))
    with lib.context(10, 2, 1) as ctx:           # (the call uses the context for its device and stream only)
        ctx.loo(w, x[:64], t[:64])               # untimed: the first launches load the code objects
        t0 = time.perf_counter()
        res = ctx.loo(w, x, t)
        out["loo_call_seconds"] = time.perf_counter() - t0
        ctx.kernel_time("enable")                # (a call of its own: the event timers are kept out of the wall time above)
        ctx.kernel_time("reset")
        again = ctx.loo(w, x, t)
        for name, key in STAGES:
            s, k = ctx.kernel_time(key)
            out[name + "_device_seconds"], out[name + "_launch_groups"] = s, k
        ctx.kernel_time("disable")
    blocks = -(-R // min(R, 64))
    out.update(column_blocks=blocks, device_seconds_per_block=sum(out[name + "_device_seconds"] for name, _ in STAGES) / blocks,
               repeat_bit_equal=bool(all(np.array_equal(res[k], again[k], equal_nan=True) for k in _capi.LOO_POINTWISE)),
               elpd_loo=res["totals"]["elpd_loo"], se_elpd_loo=res["totals"]["se_elpd_loo"], p_loo=res["totals"]["p_loo"],
               elpd_waic=res["totals"]["elpd_waic"], k_mid=res["k_mid"], k_high=res["k_high"], k_max=float(np.nanmax(res["pareto_k"])),
               tail_len=int(_capi.loo_plan([N])[0][0]))
    Rt = min(R, torch_rows)
    chunk = max(1, (1 << 30) // (8 * N))
    xd, td = torch.from_numpy(x[:Rt]).to(dev), torch.from_numpy(t[:Rt]).to(dev)
    w2 = w.reshape(N, D)
    torch_reduction(w2[:4096], xd[:chunk], td[:chunk], chunk, 16)      # untimed: rocBLAS, the sort and the element-wise kernels load
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    lppd, pw, _ = torch_reduction(w2, xd, td, chunk, out["tail_len"])
    torch.cuda.synchronize()
    out.update(torch_seconds=time.perf_counter() - t0, torch_rows=Rt, torch_chunk_rows=chunk,
               torch_scope="loglik, moments, sort and tail sum per chunk; no Pareto fit")
    out["max_abs_diff_lppd"] = float(np.abs(lppd.cpu().numpy() - res["lppd"][:Rt]).max())
    out["max_abs_diff_p_waic"] = float(np.abs(pw.cpu().numpy() - res["p_waic"][:Rt]).max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=CASES, required=True)
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--chains", type=int, default=8192)
    ap.add_argument("--draws", type=int, default=500)
    ap.add_argument("--torch-rows", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loo_bench.jsonl"))
    a = ap.parse_args()
    line = json.dumps(measure(a.case, a.rows, a.chains, a.draws, a.torch_rows))
    print(line, flush=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
