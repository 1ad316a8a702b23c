"""Case lists and input builders of the block-size and edge tests of the Gibbs, IWLS and AMH samplers: tests/test_sampler_edges_cpu.py
checks every condition that concerns the NumPy restatements alone (stability, coverage of the m/s bins, decision margins, the capped
row, saturation in chain 32), tests/test_gpu_{gibbs,iwls,amh}.py run the same inputs on the device.  A reference is computed once per
process, shared by the tests that need it and never modified afterwards (its arrays are read-only).

All inputs are `synthetic_logreg`, bundled data and Philox streams; seeds were selected on the restatements, before any device run."""
import os

import numpy as np

import test_gibbs_cpu as G
from conftest import GOLDEN, rel_err
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg
from test_amh_cpu import amh_numpy, philox_draws
from test_gibbs_cpu import PhiloxDraws, gibbs_numpy
from test_iwls_cpu import iwls_numpy, philox_iwls_draws

ULP = 1 + 2.0 ** -52
U_MAX = 1 - 2.0 ** -53          # the largest double below 1


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


# ---- Gibbs, part 1: every block count (NB = (D + 15) / 16) and the shape edges ----------------------------------------------------------
# (M, D, iterations).  NB = 2: D 17, 24, 31, 32; D == DP: 16, 32, 48; D = 1; M < 16, = 16, = 17 (the sweep's 16-row blocks, k_gibbs_b's
# 8-row stride), M = 256 / 257 (a k_gibbs_mix / k_gibbs_init block)
GIBBS_EDGE_CASES = [(300, 17, 2), (200, 24, 2), (257, 32, 2), (256, 16, 2), (120, 48, 2), (33, 31, 2), (17, 1, 3), (16, 3, 3), (3, 2, 3),
                    (15, 5, 3), (100, 1, 3)]
GIBBS_EDGE_SEED = 101           # data seed = stream seed; 102 and 103 fail the stability criterion for (200, 24) and (256, 16)
GIBBS_EDGE_CHAINS = 4


class OneUlpOff(PhiloxDraws):
    def u_init(self):
        return super().u_init() * ULP


def philox_tapes(dr, attempts):
    """the replay entry point's five tapes from the sampler's own Philox streams, given the attempts (n, T, N) every row consumes"""
    n, T, N = attempts.shape
    off = np.concatenate([np.zeros((n, T, 1), np.int64), np.cumsum(attempts, axis=2)], axis=2)
    tot = attempts.sum(axis=2)                                          # (n, T) attempts per iteration
    off = off + np.concatenate([np.zeros((n, 1), np.int64), np.cumsum(tot, axis=1)[:, :-1]], axis=1)[:, :, None]
    ks = np.zeros((n, int(tot.sum(axis=1).max()), 3))
    for it in range(T):
        for a in range(int(attempts[:, it].max())):
            Y, Ua, Ub = dr.ks(it, a, None)
            c, j = np.nonzero(attempts[:, it] > a)
            ks[c, off[c, it, j] + a] = np.stack([Y[c, j], Ua[c, j], Ub[c, j]], axis=1)
    return (dr.u_init(), np.stack([dr.u_sweep(i) for i in range(T)], axis=1), np.stack([dr.T(i) for i in range(T)], axis=1), ks, off)


_gibbs_edge = {}


def gibbs_edge_case(M, D, T):
    """dict(XX, t, draws, ref (gibbs_numpy on the Philox streams of chains 0..3), own (the restatement's beta against itself with the
    initial uniforms one ulp off: the criterion of DESIGN section 8d))"""
    key = (M, D, T)
    if key not in _gibbs_edge:
        XX, t = synthetic_logreg(M, D, GIBBS_EDGE_SEED)
        ids = np.arange(GIBBS_EDGE_CHAINS)
        dr = PhiloxDraws(GIBBS_EDGE_SEED, ids, M, D)
        ref = _freeze(gibbs_numpy(XX, t, T, dr, n=len(ids)))
        off = gibbs_numpy(XX, t, T, OneUlpOff(GIBBS_EDGE_SEED, ids, M, D), n=len(ids))
        _gibbs_edge[key] = dict(XX=XX, t=t, draws=dr, ref=ref, own=rel_err(off["beta"], ref["beta"]))
    return _gibbs_edge[key]


# ---- Gibbs, part 2: the truncated normal between the tapes' range (|m/s| <= 2.4) and the tail form (m/s > 25) ------------------------------
# The intercept-dominated data set of the far-tail test; chain c starts every label-0 row at the uniform Phi(-z0_c), so that B_0 goes
# to about -0.8 z0_c and the label-1 rows are drawn at m/s of about 0.85 z0_c in the first sweep (measured on the restatement; about
# 0.2 z0_c in the second: the chains relax at once), the label-0 rows at large negative m/s.
TN_M, TN_D, TN_T, TN_SEED = 100, 2, 3, 5
TN_Z0 = [2.5, 3.2, 4.0, 5.0, 6.5, 8.0, 10.0, 12.0, 14.0, 16.0, 18.0, 20.0, 22.0, 24.0, 25.0, 25.4, 25.8, 26.2, 26.5, 26.8, 27.1, 27.5, 29.0,
         31.0]
TN_BINS = [(2.4, 5.0, 20), (5.0, 10.0, 20), (10.0, 15.0, 20), (15.0, 20.0, 20), (20.0, 24.0, 20), (24.0, 25.0, 5), (25.0, 26.0, 5),
           (26.0, 30.0, 0), (-25.0, -15.0, 0), (-40.0, -25.0, 0)]          # (lo, hi], draws required
TN_BELOW, TN_BELOW_MIN = -15.0, 20                                          # and at least 20 draws below m/s = -15
# the last iteration's uniforms of two rows of each label in two chains (row % 10 == 0: label 1): the clamps and the ends of U
TN_EXTREME_CHAINS = (3, 13)                                                 # z0 = 5 and 24
TN_EXTREME_U = {3: {10: 1e-300, 20: U_MAX, 11: 2.0 ** -53, 12: 0.5}, 13: {10: 2.0 ** -53, 20: 0.5, 11: 1e-300, 12: U_MAX},
                22: {10: 1e-300, 20: U_MAX},                                # (beside them chain 22, z0 = 29: both ends in the tail form,
                5: {11: 1e-310}, 16: {12: 5e-324}}                          # and two subnormal uniforms on label-0 rows: p = U Phi(-m/s) < TINY)


def tn_data():
    XX = np.c_[np.ones(TN_M), np.random.RandomState(3).randn(TN_M)]
    t = (np.arange(TN_M) % 10 == 0).astype(np.float64)
    return XX, t


class TailDraws(PhiloxDraws):
    """the Philox streams with the initial uniform of every label-0 row of chain c at u0[c]; extreme: {chain: {row: U}} written over the
    sweep's uniforms of iteration `last`; ulp: the initial uniforms one ulp off"""
    def __init__(self, seed, chains, t, u0, extreme=None, last=-1, ulp=False):
        super().__init__(seed, chains, len(t), TN_D)
        self.lab0, self.u0, self.extreme, self.last, self.ulp = np.asarray(t).reshape(-1) == 0, np.asarray(u0, dtype=np.float64), extreme or {}, last, ulp

    def u_init(self):
        u = super().u_init().copy()
        u[:, self.lab0] = self.u0[:, None]
        return u * ULP if self.ulp else u

    def u_sweep(self, it):
        u = super().u_sweep(it)
        if it == self.last:
            u = u.copy()
            for c, rows in self.extreme.items():
                for j, v in rows.items():
                    u[c, j] = v
        return u


def record_truncnorm(run):
    """run() with every call of the restatement's truncnorm_neg recorded: returns (run's result, [(m, s, U) per call])"""
    calls = []
    orig = G.truncnorm_neg

    def recording(U, Uc, m, s):
        calls.append(tuple(np.array(np.broadcast_arrays(*[np.asarray(v, dtype=np.float64) for v in (m, s, U)]))))
        return orig(U, Uc, m, s)

    G.truncnorm_neg = recording
    try:
        out = run()
    finally:
        G.truncnorm_neg = orig
    return out, calls


def tn_reference(XX, t, dr, n, T):
    """gibbs_numpy on dr, with m, s (n, N) of every row's last draw (as given to truncnorm_neg: the mirrored m for label 1) and
    a (n, T N): m/s of every call of the sweeps; p_last (n, N): p = U Phi(-m/s) of the last draw as the two-tail form computes it,
    before its clamp at TINY (NaN where the draw took the tail form)"""
    ref, calls = record_truncnorm(lambda: gibbs_numpy(XX, t, T, dr, n=n))
    N = XX.shape[0]
    sweep = calls[1:]                                                   # (the first call is the initial Z: m = 0, s = 1)
    assert len(sweep) == T * N
    ref["m_last"] = np.stack([m for m, s, U in sweep[-N:]], axis=1)
    ref["s_last"] = np.stack([s for m, s, U in sweep[-N:]], axis=1)
    ref["a_calls"] = np.stack([m / s for m, s, U in sweep], axis=1)
    a = ref["m_last"] / ref["s_last"]
    ref["p_last"] = np.where(a > G.TAIL, np.nan, np.stack([U for m, s, U in sweep[-N:]], axis=1) * G._Phi(-a))
    return _freeze(ref)


def tn_bin_of(a):
    """index into TN_BINS of every m/s, -1 outside"""
    a = np.asarray(a)
    out = np.full(a.shape, -1)
    for i, (lo, hi, _) in enumerate(TN_BINS):
        out[(a > lo) & (a <= hi)] = i
    return out


def tn_tolerance(ref):
    """|Z_dev - Z_ref| <= 1e-8 |Z_ref| + 1e-12 (|m| + s): the project's Z bound per element, plus the rounding of the sum m + s y when
    m comes from differently ordered sums"""
    return 1e-8 * np.abs(ref["Z"]) + 1e-12 * (np.abs(ref["m_last"]) + ref["s_last"])


_tn = {}


def tn_extreme_mask(n):
    mask = np.zeros((n, TN_M), bool)
    for c, rows in TN_EXTREME_U.items():
        mask[c, list(rows)] = True
    return mask


def tn_mid_case(T=TN_T):
    """the batch of part 2 run for T iterations (the T = 1 run is the first iteration of the T = 3 one, up to the extreme uniforms,
    which are written into the last iteration of each): dict(XX, t, draws, ref, extreme (n, N) bool: the elements of Z drawn at an extreme uniform,
    own: the largest relative move of an element of Z with the initial uniforms one ulp off (without the extreme uniforms: where U is
    the last double below 1 the draw is the rounding of m + s y, by design), own_extreme: the move of the extreme elements in units of
    tn_tolerance)"""
    if ("mid", T) not in _tn:
        XX, t = tn_data()
        n = len(TN_Z0)
        u0 = G._Phi(-np.asarray(TN_Z0))
        mk = lambda extreme, ulp: TailDraws(TN_SEED, np.arange(n), t, u0, extreme, T - 1, ulp)
        dr = mk(TN_EXTREME_U, False)
        ref = tn_reference(XX, t, dr, n, T)
        plain, off = (gibbs_numpy(XX, t, T, mk(None, ulp), n=n) for ulp in (False, True))
        own = float(np.max(np.abs(off["Z"] - plain["Z"]) / np.abs(plain["Z"])))
        ext = tn_extreme_mask(n)
        offx = gibbs_numpy(XX, t, T, mk(TN_EXTREME_U, True), n=n)
        own_extreme = float((np.abs(offx["Z"] - ref["Z"]) / tn_tolerance(ref))[ext].max())
        _tn["mid", T] = dict(XX=XX, t=t, draws=dr, ref=ref, own=own, own_extreme=own_extreme, extreme=ext, n=n, T=T, plain_capped=plain["capped"])
    return _tn["mid", T]


def tn_far_case(T=TN_T):
    """the far-tail test's batch: three chains, every label-0 row started at the uniform 1e-300 (Z_j = -37)"""
    if ("far", T) not in _tn:
        XX, t = tn_data()
        n = 3
        dr = TailDraws(TN_SEED, np.arange(n), t, np.full(n, 1e-300))
        _tn["far", T] = dict(XX=XX, t=t, draws=dr, ref=tn_reference(XX, t, dr, n, T), n=n, T=T)
    return _tn["far", T]


def tn_report(Zdev, ref):
    """error / tolerance of every element of Z, its worst value per m/s bin of the row's last draw as {bin: (ratio, count)}"""
    ratio = np.abs(Zdev - ref["Z"]) / tn_tolerance(ref)
    b = tn_bin_of(ref["m_last"] / ref["s_last"])
    out = {}
    for i, (lo, hi, _) in enumerate(TN_BINS):
        if np.any(b == i):
            out["(%g, %g]" % (lo, hi)] = (float(ratio[b == i].max()), int((b == i).sum()))
    if np.any(b < 0):
        out["other"] = (float(ratio[b < 0].max()), int((b < 0).sum()))
    return ratio, out


# ---- Gibbs, part 3: a row that reaches the attempt bound ---------------------------------------------------------------------------------
CAP_M, CAP_D, CAP_N, CAP_T, CAP_SEED = 60, 3, 3, 3, 9
CAP_CHAIN, CAP_ROW, CAP_IT = 1, 7, 1


class CappedDraws(PhiloxDraws):
    """the second uniform of every attempt of one row of one chain in one iteration at the largest double below 1: both series tests
    reject it, the row reaches GIBBS_MAX_ATTEMPTS and keeps its last proposal"""
    def ks(self, it, a, active):
        Y, Ua, Ub = super().ks(it, a, active)
        if it == CAP_IT:
            Ub = Ub.copy()
            Ub[CAP_CHAIN, CAP_ROW] = U_MAX
        return Y, Ua, Ub


def capped_case():
    if "cap" not in _tn:
        XX, t = synthetic_logreg(CAP_M, CAP_D, CAP_SEED)
        ids = np.arange(CAP_N)
        dr, plain = CappedDraws(CAP_SEED, ids, CAP_M, CAP_D), PhiloxDraws(CAP_SEED, ids, CAP_M, CAP_D)
        _tn["cap"] = dict(XX=XX, t=t, draws=dr, plain_draws=plain, ref=_freeze(gibbs_numpy(XX, t, CAP_T, dr, n=CAP_N)),
                          plain=_freeze(gibbs_numpy(XX, t, CAP_T, plain, n=CAP_N)))
    return _tn["cap"]


# ---- IWLS: the missing block counts and the 33rd chain ------------------------------------------------------------------------------------
# (M, D, n, T, B, seed), data seed = stream seed.  NB = 3: D 40, 48, 33; D == DP: 16, 48; D = 1; n = 33: the second, partly filled
# 32-chain block of k_iwls_sat
IWLS_EDGE_CASES = [(500, 40, 33, 12, 6, 41), (300, 48, 3, 12, 6, 42), (200, 16, 3, 20, 10, 43), (100, 1, 3, 30, 15, 44),
                   (255, 33, 2, 12, 6, 45), (40, 17, 3, 12, 6, 46)]
IWLS_MARGIN = 1e-6
IWLS_SAT_N, IWLS_SAT_T, IWLS_SAT_B, IWLS_SAT_SEED = 33, 120, 60, 51      # australian, compat


def iwls_reference(XX, t, n, T, seed, compat):
    """iwls_numpy on the Philox streams of chains 0..n-1, with u (n, T), the uniform of every iteration"""
    draws = philox_iwls_draws(seed, np.arange(n), XX.shape[1])
    us = []

    def recording(it, L, mean):
        wp, u = draws(it, L, mean)
        us.append(u)
        return wp, u

    ref = iwls_numpy(XX, t, T, recording, n=n, compat=compat)
    ref["u"] = np.stack(us, axis=1)
    return _freeze(ref)


def iwls_margins(ref):
    """the distance of the closest decision from its threshold: (min |ratio|, min |ratio - log u| over the iterations that read u);
    a saturated proposal (ratio NaN) is no decision on a threshold"""
    fin = np.isfinite(ref["ratio"])
    read = fin & ref["u_read"]
    return float(np.abs(ref["ratio"][fin]).min()), float(np.abs(ref["ratio"] - np.log(ref["u"]))[read].min())


_iwls = {}


def iwls_edge_case(case, compat):
    key = (case, compat)
    if key not in _iwls:
        M, D, n, T, B, seed = case
        XX, t = synthetic_logreg(M, D, seed)
        _iwls[key] = dict(XX=XX, t=t, ref=iwls_reference(XX, t, n, T, seed, compat))
    return _iwls[key]


def iwls_sat_case():
    if "sat" not in _iwls:
        d = np.load(os.path.join(GOLDEN, "data_australian.npz"))
        _iwls["sat"] = dict(XX=d["XX"], t=d["t"], ref=iwls_reference(d["XX"], d["t"], IWLS_SAT_N, IWLS_SAT_T, IWLS_SAT_SEED, True))
    return _iwls["sat"]


# ---- AMH: wide D and the register-tile edges of M -------------------------------------------------------------------------------------------
# id: (chains, M, D, T, B, seed, (NT, R) of the instantiation of k_amh that amh_shape (csrc/plan.h) and AMH_SWITCH select);
# KW = (256 + NT - 1) / NT coordinates per thread
AMH_EDGE_CASES = {
    "nt64_d256": (1024, 300, 256, 6, 3, 61, (64, 8)),          # KW 4, every lane owns four coordinates
    "nt64_d129_odd": (1024, 250, 129, 6, 3, 62, (64, 4)),      # lane 0 owns three coordinates, the others two; half a Box-Muller pair
    "nt256_d200": (3, 400, 200, 8, 4, 63, (256, 2)),           # coordinates on waves 1-3
    "nt256_d65": (3, 350, 65, 8, 4, 64, (256, 2)),
    "nt64_m1024": (1024, 1024, 4, 10, 5, 65, (64, 16)),        # R = 16 full
    "m1025": (1024, 1025, 4, 10, 5, 66, (256, 8)),             # one row more: 256 threads per chain
    "m12288": (3, 12288, 3, 10, 5, 67, (256, 48)),             # AMH_MAX_ONCHIP_ROWS: R = 48 full
    "m12289": (3, 12289, 3, 10, 5, 68, (256, 0)),              # the first streamed size
}


def amh_follow(n):
    """the chain ids the restatement follows: all of a small batch; of a large one the first, the last and 16 spread over the batch"""
    if n <= 64:
        return np.arange(n)
    return np.unique(np.concatenate([[0, n - 1], np.linspace(1, n - 2, 16).astype(int)]))


_amh = {}


def amh_edge_case(name):
    if name not in _amh:
        n, M, D, T, B, seed, _ = AMH_EDGE_CASES[name]
        XX, t = synthetic_logreg(M, D, seed)
        ids = amh_follow(n)
        _amh[name] = dict(XX=XX, t=t, ids=ids, ref=_freeze(amh_numpy(XX, t, T, B, philox_draws(seed, ids, D), n=len(ids))))
    return _amh[name]
