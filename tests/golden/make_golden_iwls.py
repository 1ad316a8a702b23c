#!/usr/bin/env python3
"""Golden tapes for the IWLS Metropolis-Hastings sampler (code/iwls.py): runs the reference's iwls under sys.settrace in the build
container, records every np.random.multivariate_normal / np.random.uniform draw, and per iteration the proposal, its LJL, the two
proposal log-densities, the ratio, the decision, and beta, current_mean and current_LJL after the update; also the initial mean, LJL and
covariance and beta_saved.  Data only; see make_golden.py.

    python tests/golden/make_golden_iwls.py
"""
import contextlib
import io
import os
import sys

import numpy as np

REF = "/root/reference/code"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import iwls as ref_iwls  # noqa: E402  (the reference)

from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg  # noqa: E402
from make_golden import save  # noqa: E402

# source lines of code/iwls.py that are traced, found by their text so that a changed reference fails loudly
LOOP_START = 'print("--- Iterating...")'
ITER_END = "if i >= burn_in:"


def _line(frag):
    src = open(os.path.join(REF, "iwls.py")).read().splitlines()
    hits = [i + 1 for i, s in enumerate(src) if s.strip() == frag]
    assert len(hits) == 1, (frag, hits)
    return hits[0]


def _f(x):
    return float(np.ravel(x)[0])


class Rec:
    def __init__(self):
        self.l_start, self.l_end = _line(LOOP_START), _line(ITER_END)
        self.init, self.iters, self.draws = None, [], []

    def tracer(self, frame, event, arg):
        return self.local if frame.f_code.co_name == "iwls" else None

    def local(self, frame, event, arg):
        if event != "line":
            return self.local
        L = frame.f_locals
        if frame.f_lineno == self.l_start:
            self.init = (L["current_mean"].copy(), _f(L["current_LJL"]), L["current_cov"].copy())
        elif frame.f_lineno == self.l_end:
            self.iters.append(dict(w=L["beta"].copy(), mean=L["current_mean"].copy(), ljl=_f(L["current_LJL"]), accepted=int(L["accepted"]),
                                   ljl_prop=_f(L["proposed_LJL"]), q_fwd=_f(L["prob_new_given_old"]), q_rev=_f(L["prob_old_given_new"]),
                                   ratio=_f(L["ratio"])))
        return self.local


@contextlib.contextmanager
def recording_draws(rec):
    o_mvn, o_uniform = np.random.multivariate_normal, np.random.uniform

    def mvn(*a, **k):
        v = o_mvn(*a, **k)
        rec.draws.append(("mvn", np.array(v, dtype=np.float64)))
        return v

    def uniform(*a, **k):
        v = o_uniform(*a, **k)
        rec.draws.append(("uniform", float(v)))
        return v

    np.random.multivariate_normal, np.random.uniform = mvn, uniform
    try:
        yield
    finally:
        np.random.multivariate_normal, np.random.uniform = o_mvn, o_uniform


def capture(XX, t, seed, n_iter, burn_in):
    rec = Rec()
    np.random.seed(seed)
    buf = io.StringIO()
    t = np.asarray(t, dtype=np.float64).reshape(-1, 1)   # main.py's (N, 1) labels: iwls.py:34,60 need the column
    with recording_draws(rec), contextlib.redirect_stdout(buf), np.errstate(all="ignore"):
        sys.settrace(rec.tracer)
        try:
            beta_saved, _ = ref_iwls.iwls(XX, t, max_iter=n_iter, burn_in=burn_in)
        finally:
            sys.settrace(None)
    T, D = n_iter, XX.shape[1]
    assert len(rec.iters) == T
    w_prop = np.zeros((T, D)); u = np.full(T, np.nan)
    i = 0
    for it in range(T):
        k, v = rec.draws[i]; assert k == "mvn"; w_prop[it] = v; i += 1
        if i < len(rec.draws) and rec.draws[i][0] == "uniform":
            u[it] = rec.draws[i][1]; i += 1
    assert i == len(rec.draws)
    acc = np.diff(np.array([0] + [r["accepted"] for r in rec.iters])).astype(np.int8)
    g = dict(seed=np.int64(seed), n_iter=np.int64(n_iter), burn_in=np.int64(burn_in), w_prop=w_prop, u=u, accepted=acc,
             mean0=rec.init[0], ljl0=np.float64(rec.init[1]), cov0=rec.init[2], beta_saved=beta_saved)
    for key in ("w", "mean"):
        g[key] = np.stack([r[key] for r in rec.iters])
    for key in ("ljl", "ljl_prop", "q_fwd", "q_rev", "ratio"):
        g[key] = np.array([r[key] for r in rec.iters])
    return g


def main():
    for ds, seed, n_iter, burn_in in (("australian", 51, 200, 100), ("german", 52, 150, 100), ("heart", 53, 200, 100),
                                      ("pima", 54, 200, 100), ("ripley", 55, 250, 150)):
        d = np.load(os.path.join(HERE, "data_%s.npz" % ds))
        save("iwls_" + ds, **capture(d["XX"], d["t"], seed, n_iter, burn_in))
    XX, t = synthetic_logreg(3000, 64, 5)
    g = capture(XX, t, 56, 30, 20)
    g.update(M=np.int64(3000), D=np.int64(64), data_seed=np.int64(5))
    save("iwls_syn_m3000_d64", **g)
    # One row far out along a column of its own (x = 1000, t = 1): once that row saturates it no longer constrains the proposal along the
    # column, whose spread then comes from the prior - proposals with f > 709.78, where exp(f) overflows and the reference's LJL is -inf.
    # The data are stored with the tape.
    XX, t = synthetic_logreg(100, 4, 6)
    XX = np.hstack([XX, np.zeros((100, 1))]); XX[0, -1] = 1000.0
    t = np.array(t, dtype=np.float64).reshape(-1); t[0] = 1.0
    g = capture(XX, t, 59, 300, 200)
    g.update(XX=XX, t=t)
    save("iwls_syn_m100_d5_outlier", **g)


if __name__ == "__main__":
    main()
