#!/usr/bin/env python3
"""Golden tapes for the adaptive Metropolis sampler (code/metropolis.py): runs the reference's AMH under sys.settrace in the build
container, records every np.random.normal / np.random.rand draw, the decision of every proposal, and w, CurrentLJL and ProposalSD
after every iteration (after the adaptation).  Data only; see make_golden.py.

    python tests/golden/make_golden_amh.py
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

import metropolis as ref_amh  # noqa: E402  (the reference)

from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg  # noqa: E402
from make_golden import save  # noqa: E402

# source lines of code/metropolis.py that are traced, found by their text so that a changed reference fails loudly
ACCEPT = "CurrentLJL = ProposedLJL"
ITER_END = "if IterationNum == BurnIn:"


def _line(frag):
    src = open(os.path.join(REF, "metropolis.py")).read().splitlines()
    hits = [i + 1 for i, s in enumerate(src) if s.strip() == frag]
    assert len(hits) == 1, (frag, hits)
    return hits[0]


class Rec:
    def __init__(self):
        self.l_acc, self.l_end = _line(ACCEPT), _line(ITER_END)
        self.accepted, self.iters, self.draws = [], [], []

    def tracer(self, frame, event, arg):
        return self.local if frame.f_code.co_name == "AMH" else None

    def local(self, frame, event, arg):
        if event != "line":
            return self.local
        L = frame.f_locals
        if frame.f_lineno == self.l_acc:
            self.accepted.append((int(L["IterationNum"]), int(L["d"])))
        elif frame.f_lineno == self.l_end:
            self.iters.append((L["w"].copy().ravel(), float(np.ravel(L["CurrentLJL"])[0]), L["ProposalSD"].copy().ravel()))
        return self.local


@contextlib.contextmanager
def recording_draws(rec):
    o_normal, o_rand = np.random.normal, np.random.rand

    def normal(*a, **k):
        v = o_normal(*a, **k)
        rec.draws.append(("normal", float(v)))
        return v

    def rand(*a):
        v = o_rand(*a)
        rec.draws.append(("rand", float(v)))
        return v

    np.random.normal, np.random.rand = normal, rand
    try:
        yield
    finally:
        np.random.normal, np.random.rand = o_normal, o_rand


def capture(XX, t, seed, n_iter, burn_in):
    rec = Rec()
    np.random.seed(seed)
    buf = io.StringIO()
    with recording_draws(rec), contextlib.redirect_stdout(buf), np.errstate(all="ignore"):
        sys.settrace(rec.tracer)
        try:
            wSaved, _ = ref_amh.AMH(XX, t, NumOfIterations=n_iter, BurnIn=burn_in)
        finally:
            sys.settrace(None)
    T, D = n_iter, XX.shape[1]
    assert len(rec.iters) == T
    z = np.zeros((T, D)); u = np.full((T, D), np.nan); acc = np.zeros((T, D), dtype=np.int8)
    i = 0
    for it in range(T):
        for d in range(D):
            k, v = rec.draws[i]; assert k == "normal"; z[it, d] = v; i += 1
            if i < len(rec.draws) and rec.draws[i][0] == "rand":
                u[it, d] = rec.draws[i][1]; i += 1
    assert i == len(rec.draws)
    for it, d in rec.accepted:
        acc[it, d] = 1
    return dict(seed=np.int64(seed), n_iter=np.int64(n_iter), burn_in=np.int64(burn_in), z=z, u=u, accepted=acc,
                w=np.stack([r[0] for r in rec.iters]), ljl=np.array([r[1] for r in rec.iters]), sd=np.stack([r[2] for r in rec.iters]),
                wSaved=wSaved)


def main():
    for ds, seed, n_iter, burn_in in (("australian", 41, 220, 210), ("heart", 42, 220, 210), ("pima", 43, 120, 110),
                                      ("ripley", 44, 120, 110)):
        d = np.load(os.path.join(HERE, "data_%s.npz" % ds))
        save("amh_" + ds, **capture(d["XX"], d["t"], seed, n_iter, burn_in))
    # (x_scale: exp(f) overflows in the reference for most proposals, LJL = -inf, Ratio = -inf: u drawn, proposal rejected)
    for name, M, D, dseed, x_scale, seed, n_iter, burn_in in (("syn_m3000_d64", 3000, 64, 5, 1.0, 45, 30, 25),
                                                              ("syn_m200_d6_x300", 200, 6, 6, 300.0, 46, 120, 110)):
        XX, t = synthetic_logreg(M, D, dseed)
        g = capture(XX * x_scale, t, seed, n_iter, burn_in)
        g.update(M=np.int64(M), D=np.int64(D), data_seed=np.int64(dseed), x_scale=np.float64(x_scale))
        save("amh_" + name, **g)


if __name__ == "__main__":
    main()
