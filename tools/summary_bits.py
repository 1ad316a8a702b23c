#!/usr/bin/env python3
"""Every output of the summary kernels (adapt, ais, smc, pred, loo, diag, quant .hip.h) on fixed inputs, saved under stable names, so that
two builds of the library can be compared bit for bit: a change that leaves every floating-point sum in its order leaves every array
equal.

    RMHMC_HIP_LIB=<library> python tools/summary_bits.py OUT.npz       # the library of the tree without RMHMC_HIP_LIB
    python tools/summary_bits.py --compare A.npz B.npz                  # exit status 1 and the names where an array differs

Inputs come from fixed seeds and nothing outside the tree is read.  Shapes: N = 1, 17, 1000, 4099 draws; 1, 16, 17, 64 rows or columns
(65 for predict); one D per KS case of the draw product; P, S and lag counts that reach every tile width of diag and quant with one and
with four lag sets; every JT of the conditional-ESS dispatch; per family a NaN draw, a +-inf draw and all -inf weights.  One
phmc_warmup, one ais_run and one smc_run on a 300 x 5 problem bring the composed paths in.  Two runs are meant to be separate
processes, each under a time limit of its own, chained with &&."""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

DRAWS = ((1, 1), (1, 17), (4, 250), (1, 4099))                        # chains x samples
DS = (1, 16, 17, 32, 64, 96, 128, 160, 192, 224, 256)                # KS = 4, 4, 8, 8, 16, 24, .., 64
ROWS = (1, 16, 17, 64)
SIGN = 1 << 63


def compare(a, b):
    A, B = np.load(a), np.load(b)
    names = sorted(A.files)
    bad = [k for k in names if k not in B.files or A[k].dtype != B[k].dtype or A[k].shape != B[k].shape or A[k].tobytes() != B[k].tobytes()]
    bad += [k for k in B.files if k not in A.files]
    print("%d arrays compared, %d differ" % (len(names), len(bad)))
    for k in bad:
        print("  differs:", k)
    return 1 if bad else 0


def unkey(key):
    key = int(key)
    u = key ^ SIGN if key & SIGN else ~key & (2 ** 64 - 1)
    return np.array([u], dtype=np.uint64).view(np.float64)[0]


def spoil(w, kind):
    """a copy of w [n][S][D] with one draw made NaN ("nan") or given a +inf and a -inf entry ("inf")"""
    w = w.copy()
    flat = w.reshape(-1, w.shape[-1])
    j = flat.shape[0] // 2
    if kind == "nan":
        flat[j, -1] = np.nan
    elif kind == "inf":
        flat[j, 0] = np.inf
        flat[flat.shape[0] - 1, -1] = -np.inf
    return w


def main(path):
    import torch
    from riemannhamiltonianmontecarlo_amd import _capi
    from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg
    lib = _capi.load_hip_library()
    devc = torch.device("cuda", 0)
    out = {}

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(devc)

    def put(name, v):
        assert name not in out, name
        out[name] = np.ascontiguousarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v))

    def loo_pieces(ctx, name, ll):
        part = ctx.loo_moments(ll)
        put(name + "/moments", part)
        ph = part.cpu().numpy()
        Cn = ph.shape[1]
        tl, rank0 = _capi.loo_plan(ph[0].astype(np.int64))
        cut = np.full(Cn, np.nan)
        if (rank0 >= 0).any():
            prefix = np.zeros((1, Cn), dtype=np.uint64)
            rank = rank0.reshape(1, Cn).copy()
            for r in range(_capi.QUANT_ROUNDS):
                _capi.quant_step([ctx.quant_hist(ll, r, prefix if r else None, 1)], r, prefix, rank)
            for c in range(Cn):
                if tl[c] >= 5:
                    cut[c] = unkey(prefix[0, c])
        sp = ctx.loo_split(ll, cut, ph[4], tl)
        counts = sp["counts"].cpu().numpy()
        tail = sp["tail"].cpu().numpy()
        srt = np.zeros_like(tail)                      # the slots of a tail are filled in no order: compared as a sorted set
        for c in range(Cn):
            k = int(min(counts[0, c], tl[c], tail.shape[1]))
            srt[c, :k] = np.sort(tail[c, :k])
        put(name + "/split_counts", counts)
        put(name + "/split_body", sp["body"])
        put(name + "/split_tail_sorted", srt)
        put(name + "/fit", ctx.loo_fit(sp["tail"], sp["counts"], cut, ph[4], tl))

    with lib.context(10, 2, 1) as ctx:                 # (these calls use the context for its device and stream only)
        # ---- pooled covariance: P at the column groups of a lane and the tiles of the second pass
        for n, S in DRAWS:
            for P in (1, 16, 17, 64, 65, 130, 256):
                rs = np.random.RandomState(1000 * P + n * S)
                x = rs.randn(n, S, P) + 1e3
                put("cov/N%d_P%d" % (n * S, P), ctx.cov_partial(dev(x)))
                if n * S == 1000:
                    for kind in ("nan", "inf"):
                        put("cov/N1000_P%d_%s" % (P, kind), ctx.cov_partial(dev(spoil(x, kind))))
        # ---- importance weights and the conditional ESS: every JT (1, 4, 16, 32) with and without padding
        for N in (1, 17, 1000, 4099, 70000):
            rs = np.random.RandomState(N)
            lw = 5.0 * rs.randn(N)
            ll = -np.abs(30.0 * rs.randn(N))
            variants = dict(plain=(lw, ll))
            if N > 1:
                a, b = lw.copy(), ll.copy()
                a[N // 3] = np.nan
                b[N // 2] = -np.inf
                a[N - 1] = -np.inf
                variants["nan_inf"] = (a, b)
                c = lw.copy()
                c[0] = np.inf
                variants["pinf"] = (c, ll)
            variants["all_ninf"] = (np.full(N, -np.inf), ll)
            for tag, (a, b) in variants.items():
                da, db = dev(a), dev(b)
                put("ais/N%d_%s" % (N, tag), ctx.ais_partial(da))
                for J in (1, 3, 4, 9, 16, 20, 32):
                    delta = np.linspace(0.002, 0.3, J)
                    put("smc_cess/N%d_%s_J%d" % (N, tag, J), ctx.smc_cess(da, db, delta))
                r = ctx.smc_choose_delta(da, db, 0.7, 0.9)
                put("smc_choose/N%d_%s" % (N, tag), np.array([r["delta"], r["frac"], float(r["flags"])]))
        # ---- predictive probabilities and the log-likelihood matrix: every KS, every row edge
        for D in DS:
            for n, S in DRAWS:
                N = n * S
                rs = np.random.RandomState(100 * D + N)
                w = rs.randn(n, S, D) * (3.0 / np.sqrt(D))
                x = rs.randn(65, D)
                t = (rs.rand(65) < 0.5).astype(np.float64)
                ws = dict(plain=w)
                if N == 1000:
                    ws.update(nan=spoil(w, "nan"), inf=spoil(w, "inf"))
                for tag, wv in ws.items():
                    dw = dev(wv)
                    for R in ROWS + (65,):
                        if tag != "plain" and R not in (17, 65):
                            continue
                        put("pred/D%d_N%d_R%d_%s" % (D, N, R, tag), ctx.predict_partial(dw, x[:R]))
                        put("pred/D%d_N%d_R%d_%s_labels" % (D, N, R, tag), ctx.predict_partial(dw, x[:R], t[:R]))
                    for Cn in ROWS:
                        if tag != "plain" and Cn != 17:
                            continue
                        name = "loo/D%d_N%d_C%d_%s" % (D, N, Cn, tag)
                        ll = ctx.loo_loglik(dw, x[:Cn], t[:Cn])
                        put(name + "/loglik", ll)
                        if D in (17, 256) or Cn == 17:
                            loo_pieces(ctx, name, ll)
                    if N in (1000, 4099) and D in (17, 64):
                        r = ctx.loo(dw, x, t, cols_per_block=0 if D == 17 else 16)
                        for k in _capi.LOO_POINTWISE + ("partial", "fit", "body", "draws_used"):
                            put("loo_whole/D%d_N%d_%s/%s" % (D, N, tag, k), r[k])
        # a long tail for the fit (N 70000: a tail of several hundred), and the moments of a column whose log-likelihoods are all -inf
        rs = np.random.RandomState(7)
        ll = dev(-np.abs(rs.randn(7, 10000, 5)) * 3.0)
        loo_pieces(ctx, "loo/long_tail", ll)
        ll2 = -np.abs(rs.randn(1, 1000, 3))
        ll2[:, :, 1] = -np.inf
        ll2[0, 5, 2] = np.nan
        put("loo/ninf_column/moments", ctx.loo_moments(dev(ll2)))
        # ---- diagnostics: (n, S, P, max_lag) -> tile width and lag sets 1 | 4
        for n, S, P, lag in ((33, 40, 1, None), (2, 8400, 1, None), (33, 40, 2, 7), (2, 4200, 2, None), (33, 41, 3, None), (2, 2100, 4, None),
                             (33, 40, 5, 3), (2, 1100, 8, None), (33, 40, 16, None), (2, 600, 9, None), (33, 40, 17, None), (2, 300, 32, None),
                             (33, 40, 64, None), (2, 200, 33, None), (3, 100, 70, 20), (1, 4, 1, None)):
            rs = np.random.RandomState(S + P)
            x = np.cumsum(rs.randn(n, S, P), axis=1) * 0.1 + rs.randn(n, S, P)
            name = "diag/n%d_S%d_P%d_lag%s" % (n, S, P, lag)
            put(name, ctx.diag_partial(dev(x), lag))
            if S == 40:
                for kind in ("nan", "inf"):
                    put(name + "_" + kind, ctx.diag_partial(dev(spoil(x, kind)), lag))
        # ---- quantiles: round 0 and round 1 at every tile width, two column tiles at P = 70
        for n, S in DRAWS:
            for P in (1, 2, 3, 5, 9, 17, 33, 64, 70):
                rs = np.random.RandomState(n * S + P)
                x = rs.randn(n, S, P)
                for tag, xv in (("plain", x),) + ((("nan", spoil(x, "nan")), ("inf", spoil(x, "inf"))) if n * S == 1000 else ()):
                    dx = dev(xv)
                    name = "quant/N%d_P%d_%s" % (n * S, P, tag)
                    h0 = ctx.quant_hist(dx, 0)
                    put(name + "/round0", h0)
                    m = _capi.quant_totals([h0])
                    rank, _ = _capi.quant_plan(m, [0.05, 0.5, 0.95])
                    prefix = np.zeros(rank.shape, dtype=np.uint64)
                    _capi.quant_step([h0], 0, prefix, rank)
                    put(name + "/round1", ctx.quant_hist(dx, 1, prefix))
    # ---- the composed paths on a 300 x 5 problem
    M, D, n = 300, 5, 64
    XX, t = synthetic_logreg(M, D, 1)
    H = 0.25 * XX.T @ XX
    with lib.context(M, D, n) as ctx:
        ctx.set_data(XX, t)
        ctx.phmc_set_mass(None)
        r = ctx.phmc_warmup([6] * 4, [0, 1, 1, 0], L=5, eps0=0.1, min_rows=30, seed=4)
        for k in ("theta", "eps_trace", "accept_trace", "mass_updated"):
            put("warmup/" + k, r[k])
        put("warmup/step_size", np.array([r["step_size"]]))
        if r["mass"] is not None:
            put("warmup/mass", r["mass"])
    with lib.context(M, D, n) as ctx:
        ctx.set_data(XX, t)
        ctx.phmc_set_mass(None)
        r = ctx.ais_run(*_capi.ais_schedule(8), H_lik=H, L=4, eps=0.3, seed=5)
        for k in ("logw", "theta", "accept_trace", "partial"):
            put("ais_run/" + k, r[k])
    with lib.context(M, D, n) as ctx:
        ctx.set_data(XX, t)
        ctx.phmc_set_mass(None)
        r = ctx.smc_run(rho=0.9, tau=0.5, T_max=40, H_lik=H, L=4, eps=0.3, seed=6)
        for k in ("beta", "cess", "ess", "flags", "accept_trace", "logw", "theta", "partial"):
            put("smc_run/" + k, r[k])
        put("smc_run/log_z", np.array([r["log_z"], r["se"]]))
    np.savez(path, **out)
    print("%d arrays saved to %s (%s)" % (len(out), path, lib.version()))
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1]))
