#!/usr/bin/env python3
"""Golden tapes for the auxiliary-variable Gibbs sampler (code/gibbs_sampler.py): runs the reference's auxiliary_gibbs (needs the
reference tree and SciPy, like make_golden.py) and records, per tape, the uniform behind every scipy.stats.truncnorm.rvs call (one uniform of the global
stream per call, checked on every call), the T of every multivariate_normal call, the (normal, uniform, uniform) triple of every
mixing-weight attempt with per-row offsets, beta, B (before the T term) and the attempts per row after every iteration, Z and the
mixing weights after the last one.  Data only; see make_golden.py.

    python tests/golden/make_golden_gibbs.py              # the tapes and the truncated-normal fixture
    python tests/golden/make_golden_gibbs.py --moments    # gibbs_ripley_moments.npz: 12 long runs of the reference (minutes)
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

import gibbs_sampler as ref_gibbs  # noqa: E402  (the reference)

from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg  # noqa: E402
from make_golden import save  # noqa: E402


class Rec:
    def __init__(self):
        self.tn = []        # (u, a, b, loc, scale, value) of every truncnorm.rvs call
        self.T = []         # T of every multivariate_normal call
        self.B = []         # B at that call
        self.beta = []      # B + L T
        self.ks = []        # (normal, uniform, uniform) of every mixing-weight attempt
        self.att = []       # attempts of every mixing_weights_sampling call
        self.frame_Z = self.frame_lam = None


@contextlib.contextmanager
def recording(rec):
    tn = ref_gibbs.stats.truncnorm
    o_rvs, o_mvn, o_mws = tn.rvs, np.random.multivariate_normal, ref_gibbs.mixing_weights_sampling
    o_normal, o_uniform = np.random.normal, np.random.uniform
    cur = []

    def rvs(a, b, loc=0, scale=1):
        st = np.random.get_state()
        rs = np.random.RandomState()
        rs.set_state(st)
        u = rs.uniform()
        v = o_rvs(a, b, loc=loc, scale=scale)
        s1, s2 = rs.get_state(), np.random.get_state()
        assert np.array_equal(s1[1], s2[1]) and s1[2:] == s2[2:], "truncnorm.rvs took more than one uniform"
        rec.tn.append((u, float(a), float(b), float(loc), float(scale), float(v)))
        return v

    def mvn(mean, cov):
        T = o_mvn(mean, cov)
        L = sys._getframe(1).f_locals
        rec.T.append(T.copy()); rec.B.append(L["B"].copy()); rec.beta.append(L["B"] + L["L"].dot(T))
        rec.frame_Z, rec.frame_lam = L["Z"], L["mix_weights"]   # mutated in place, never rebound: final values after the run
        return T

    def normal():
        v = o_normal(); cur.append(float(v)); return v

    def uniform():
        v = o_uniform(); cur.append(float(v)); return v

    def mws(r2):
        del cur[:]
        lam = o_mws(r2)
        assert len(cur) % 3 == 0
        rec.ks.extend(cur); rec.att.append(len(cur) // 3)
        return lam

    tn.rvs, np.random.multivariate_normal, ref_gibbs.mixing_weights_sampling = rvs, mvn, mws
    np.random.normal, np.random.uniform = normal, uniform
    try:
        yield
    finally:
        del tn.rvs
        np.random.multivariate_normal, ref_gibbs.mixing_weights_sampling = o_mvn, o_mws
        np.random.normal, np.random.uniform = o_normal, o_uniform


def capture(XX, t, seed, n_iter, v=100.0, tn_sample=False):
    rec = Rec()
    np.random.seed(seed)
    N, D = XX.shape
    with recording(rec), contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        saved, _ = ref_gibbs.auxiliary_gibbs(XX, t, v=v, max_iter=n_iter, burn_in=0)
    tf = np.asarray(t).reshape(-1)
    order = np.concatenate([np.where(tf == 1)[0], np.where(tf == 0)[0]])   # gibbs_sampler.py:82-93: ones first, then zeros
    tn = np.array(rec.tn)
    assert len(tn) == N * (n_iter + 1) and len(rec.att) == N * n_iter and len(rec.T) == n_iter
    u_init = np.zeros(N); u_init[order] = tn[:N, 0]
    att = np.array(rec.att, dtype=np.int64).reshape(n_iter, N)
    off = np.concatenate([[0], np.cumsum(att.ravel())]).astype(np.int64)
    ks_offset = np.stack([off[i * N:(i + 1) * N + 1] for i in range(n_iter)])
    beta = np.stack(rec.beta)
    assert np.array_equal(beta, saved)
    g = dict(seed=np.int64(seed), n_iter=np.int64(n_iter), v=np.float64(v), u_init=u_init,
             u_sweep=tn[N:, 0].reshape(n_iter, N), T=np.stack(rec.T), ks_draws=np.array(rec.ks).reshape(-1, 3), ks_offset=ks_offset,
             beta=beta, B=np.stack(rec.B), attempts=att.astype(np.int16), Z=rec.frame_Z.copy(), lam=rec.frame_lam.copy())
    if tn_sample:  # the truncated-normal calls of the last sweep themselves: m, s, label, SciPy's value
        g.update(tn_u=tn[-N:, 0], tn_m=tn[-N:, 3], tn_s=tn[-N:, 4], tn_t=(tn[-N:, 1] > -np.inf).astype(np.int8), tn_x=tn[-N:, 5])
    return g


def flip(t, frac, seed):
    t = np.array(t, dtype=np.float64)
    idx = np.random.RandomState(seed).choice(t.size, int(frac * t.size), replace=False)
    t.reshape(-1)[idx] = 1.0 - t.reshape(-1)[idx]
    return t


def _exact_truncnorm(U, m, s, lab):
    """the quantile in multiprecision arithmetic (mpmath; digits to spare for Phi(-40) = 1e-350)"""
    import mpmath as mp
    with mp.workdps(60 + int((m / s) ** 2 / 4.6)):
        U, m, s = mp.mpf(U), mp.mpf(m), mp.mpf(s)
        if lab:
            U, m = 1 - U, -m
        y = -mp.sqrt(2) * mp.erfinv(1 - 2 * U * mp.ncdf(-m / s))
        x = m + s * y
        return float(-x if lab else x)


def truncnorm_fixture():
    """SciPy's truncated normal (its ppf at U: what rvs returns, see capture) on a grid of U and m/s in [-40, 40], both labels, with the
    exact value beside it: where U is within 1e-12 of the truncated end SciPy's own value is rounding noise of m + s y (no correct digit)"""
    import scipy.stats as stats
    rs = np.random.RandomState(7)
    rows = []
    for a in np.concatenate([np.linspace(-40, 40, 41), rs.uniform(-6, 6, 40)]):
        for U in (1e-12, 0.003, 0.25, 0.5, 0.8, 0.999, 1 - 1e-12, rs.uniform()):
            for lab in (0, 1):
                s = float(np.exp(rs.uniform(-2, 2)))
                m = a * s
                lo, hi = ((0 - m) / s, np.inf) if lab else (-np.inf, (0 - m) / s)
                rows.append((U, m, s, lab, float(stats.truncnorm.ppf(U, lo, hi, loc=m, scale=s)), _exact_truncnorm(U, m, s, lab)))
    r = np.array(rows)
    save("gibbs_truncnorm", u=r[:, 0], m=r[:, 1], s=r[:, 2], t=r[:, 3].astype(np.int8), x=r[:, 4], x_exact=r[:, 5])


def one_long_run(seed):
    """(mean, std) of the 5000 saved rows, or a description of the reference's failure: the run stops with a ValueError of SciPy's when
    the scale of a row's draw is not a positive finite number (seen: lam_j = inf out of mixing_weights_sampling, whose proposal cancels to
    0 for a tiny residual)"""
    d = np.load(os.path.join(HERE, "data_ripley.npz"))
    np.random.seed(seed)
    tn = ref_gibbs.stats.truncnorm
    o_rvs = tn.rvs
    why = []

    def rvs(a, b, loc=0, scale=1):
        try:
            return o_rvs(a, b, loc=loc, scale=scale)
        except ValueError:
            L = sys._getframe(1).f_locals
            why.append("iteration %d row %d: lam %.6g h %.6g w %.6g scale %r" % (L["i"], L["j"], L["mix_weights"][L["j"]], L["H"][L["j"]],
                                                                                 L["W"][L["j"]], scale))
            raise

    tn.rvs = rvs
    try:
        with contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
            s, _ = ref_gibbs.auxiliary_gibbs(d["XX"], d["t"], v=100, max_iter=5500, burn_in=500)
    except ValueError:
        return seed, why[0]
    finally:
        del tn.rvs
    return seed, (s.mean(axis=0), s.std(axis=0))


def moments():
    """16 runs of the reference, seeds 101..116: the first 12 that complete; the failed ones are listed in the fixture"""
    import multiprocessing as mp
    seeds = list(range(101, 117))
    with mp.Pool(min(len(seeds), os.cpu_count() or 1)) as pool:
        r = pool.map(one_long_run, seeds, chunksize=1)
    good = [(sd, v) for sd, v in r if not isinstance(v, str)][:12]
    bad = [(sd, v) for sd, v in r if isinstance(v, str)]
    for sd, v in bad:
        print("seed %d: the reference stopped, %s" % (sd, v))
    assert len(good) == 12, len(good)
    save("gibbs_ripley_moments", seeds=np.array([sd for sd, _ in good], dtype=np.int64), n_iter=np.int64(5500), burn_in=np.int64(500),
         v=np.float64(100), mean=np.stack([a for _, (a, _) in good]), std=np.stack([b for _, (_, b) in good]),
         failed_seeds=np.array([sd for sd, _ in bad], dtype=np.int64))


def main():
    if "--moments" in sys.argv:
        return moments()
    if "--tapes-only" not in sys.argv:
        truncnorm_fixture()
    for ds, seed, n_iter in (("ripley", 51, 6), ("heart", 52, 6), ("pima", 53, 3), ("australian", 54, 2)):
        d = np.load(os.path.join(HERE, "data_%s.npz" % ds))
        save("gibbs_" + ds, **capture(d["XX"], d["t"], seed, n_iter, tn_sample=ds == "ripley"))
    for name, M, D, dseed, x_scale, fl, seed, n_iter in (("syn_m400_d64", 400, 64, 5, 1.0, 0.0, 55, 3),
                                                         ("syn_m300_d33", 300, 33, 6, 1.0, 0.0, 56, 3),
                                                         ("syn_m150_d5_x30", 150, 5, 7, 30.0, 0.05, 57, 6)):
        XX, t = synthetic_logreg(M, D, dseed)
        t = flip(t, fl, dseed) if fl else t
        g = capture(XX * x_scale, t, seed, n_iter)
        g.update(M=np.int64(M), D=np.int64(D), data_seed=np.int64(dseed), x_scale=np.float64(x_scale), flip=np.float64(fl))
        save("gibbs_" + name, **g)


if __name__ == "__main__":
    main()
