"""Harness of tests/test_phmc_edges_cpu.py and tests/test_gpu_phmc_edges.py: fixed-metric HMC (csrc/phmc.hip.h), its tempered form
(csrc/ais.hip.h) and the prior draws of annealed importance sampling at every chain slot of a workgroup and at the tile edges of D.

k_phmc_head, k_phmc_tail and k_tphmc_tail give a 256-thread workgroup 16 chains: wavefront wv owns the chains wv + 4 jj, jj = 0..3, and a
chain is column lane & 15 of the MFMA products with the shared matrices.  The kernels are templated on NDB = DP / 16: 1..4 for D <= 64,
and 8, 12, 16 for the large-D contexts (DP a multiple of 64), where the matrix is staged in 32-column blocks with a barrier in between and
a wavefront holds (NDB + 3) / 4 > 1 accumulators.  The tables below hold one small batch per edge; `why` says which it is there for.

References: the NumPy restatements phmc_ref.py and ais_ref.py, one chain at a time in float64.  The sampler reference chains them over
the iterations on the Philox streams of plain HMC, restated here from the streams' specification (csrc/kernels.hip.h, oracle/) and pinned
to the CPU oracle's rmhmc_hmc_sample by tests/test_phmc_edges_cpu.py.

GPU-free: tables, inputs and references.  Each reference is computed once per process, shared and read-only."""
import collections
import math
import os
import sys

import numpy as np

from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ais_ref as A  # noqa: E402
import phmc_ref as R  # noqa: E402
from test_amh_cpu import M32, _u53, philox4x32_10  # noqa: E402

ALPHA = 100.0
L, EPS = 8, 0.5                      # the transition of tests/test_gpu_phmc.py
BETAS = (None, 0.3)                  # None: phmc_transition; 0.3: tphmc_transition under the stage mass beta H + I / alpha
BLOCK_LEN_ACC = 0x40000000           # the Philox block of (u_len, u_acc)
PRIOR_ITER = 0xFFFFFFFF              # RMHMC_AIS_PRIOR_ITER (include/rmhmc_ais.h)

_cache = {}


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def ndb_of(D):
    """NDB of the instantiation a context of D columns gets (PHMC_SWITCH in csrc/rmhmc_hip.hip)"""
    return (D + 15) // 16 if D <= 64 else 4 * ((D + 63) // 64)


def x_scale(D):
    """columns of unit variance for D <= 64; rows of unit length above: with unit-variance columns the restatement's own trajectories
    overflow at eps = 0.5 for D = 128, 191, 192, 193 and 255 (H_prop = inf on the CPU as on the GPU: nothing left to compare)"""
    return 1.0 if D <= 64 else 1.0 / math.sqrt(D)


# ---- the problem and the mass of a stage -----------------------------------------------------------------------------------------------
def problem(M, D):
    """data, the restatement's mode, the metric there and its factor; H: the likelihood part of the metric"""
    key = ("problem", M, D)
    if key not in _cache:
        XX, t = synthetic_logreg(M, D, 1)
        XX = XX * x_scale(D)
        m = R.mode(XX, t)
        assert m["converged"]
        _cache[key] = _freeze(dict(M=M, D=D, XX=XX, t=t, mode=m["w"], G=m["G"], H=m["G"] - np.eye(D) / ALPHA))
    return _cache[key]


def stage(M, D, beta):
    """the problem with the mass of a stage: beta None -> the metric at the mode, centred there (tests/test_gpu_phmc.py::draws);
    otherwise beta H + I / alpha centred at the mode of the tempered target (tests/test_gpu_ais.py::tempered_draws)"""
    key = ("stage", M, D, beta)
    if key not in _cache:
        pr = problem(M, D)
        if beta is None:
            Mass, centre = pr["G"], pr["mode"]
        else:
            Mass, centre = A.stage_mass_matrix(beta, pr["H"], ALPHA), A.mode(pr["XX"], pr["t"], beta)
        _cache[key] = _freeze(dict(M=M, D=D, XX=pr["XX"], t=pr["t"], beta=beta, Mass=Mass, Lm=np.linalg.cholesky(Mass), centre=centre))
    return _cache[key]


def identity_problem(M, D, data_seed=1):
    """the same data with the identity as mass matrix: plain HMC, what the CPU oracle runs"""
    XX, t = synthetic_logreg(M, D, data_seed)
    return dict(M=M, D=D, XX=XX * x_scale(D), t=t, beta=None, Mass=None, Lm=None, centre=np.zeros(D))


def draws(st, n, seed, zero_steps=()):
    """starts from N(centre, Mass^-1), momentum normals, the two uniforms; chain 0 runs the full length, `zero_steps` none at all"""
    D = st["D"]
    rs = np.random.RandomState(seed)
    w = np.stack([st["centre"] + R.solve_upper(st["Lm"].T, rs.randn(D)) for _ in range(n)])
    z = rs.randn(n, D)
    u_len = rs.uniform(0.05, 1.0, n); u_acc = rs.uniform(0.05, 1.0, n)
    u_len[0] = 1.0
    for c in zero_steps:
        u_len[c] = 0.0
    return dict(w=w, z=z, u_len=u_len, u_acc=u_acc)


def reference(st, inp, L=L, eps=EPS):
    """the restatement's transition of the batch"""
    with np.errstate(all="ignore"):
        if st["beta"] is None:
            return R.transitions(st["XX"], st["t"], st["Lm"], inp["w"], inp["z"], inp["u_len"], inp["u_acc"], L, eps, ALPHA)
        return A.transitions(st["XX"], st["t"], st["Lm"], inp["w"], inp["z"], inp["u_len"], inp["u_acc"], L, eps, st["beta"], ALPHA)


# ---- transition tables -----------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "id M D n zero_steps why")


def _d_why(D):
    NDB, r = ndb_of(D), D % 16
    DP = 16 * NDB
    tile = "exact tiles" if D == DP else ("last tile holds %d of 16 rows" % r if DP - D < 16 else "%d padded rows" % (DP - D))
    if NDB <= 4:
        return "NDB %d: the matrix in LDS whole, one accumulator, %s" % (NDB, tile)
    return "NDB %d: %d column blocks of 32, %d accumulators (wavefront 3 owns %d row tiles), %s" % (
        NDB, DP // 32, (NDB + 3) // 4, len(range(3, NDB, 4)), tile)


# (300, D, 18): chains 0..15 fill a workgroup, so every slot jj and every wavefront carries a chain and product columns 0..15 are all in
# use; chains 16, 17 are a second workgroup with two idle wavefronts that still take part in the barriers.  Chain 5 takes no step among
# chains that do (the head's zero-step branch, phase 2 in the tails); chains 16, 17 take none: a workgroup in which no chain steps.
D_EDGES = (16, 17, 32, 47, 48, 49, 63, 127, 128, 129, 191, 192, 193, 255)
D_ZERO = (5, 16, 17)
D_CASES = [Case("d-300x%dx18" % _D, 300, _D, 18, D_ZERO, _d_why(_D)) for _D in D_EDGES]


def _n_zero(n):
    """chain 5 where the batch has it; the last chain where it is alone in its workgroup (that workgroup then starts and ends a
    transition without a step)"""
    return tuple(c for c in (5, n - 1 if n > 1 and n % 16 == 1 else None) if c is not None and c < n)


def _n_why(n, NDB):
    g, last = (n + 15) // 16, n - 16 * ((n + 15) // 16 - 1)
    return "NDB %d, %d chains: %d workgroup(s) of 16, last holds %d (%d idle wavefront(s), %d idle slot(s))" % (
        NDB, n, g, last, max(0, 4 - last), 16 - last)


N_CASES = [Case("n-200x20x%d" % _n, 200, 20, _n, _n_zero(_n), _n_why(_n, 2)) for _n in (1, 15, 16, 17, 32, 33, 65)]
N_CASES += [Case("n-300x129x%d" % _n, 300, 129, _n, _n_zero(_n), _n_why(_n, 12)) for _n in (16, 17, 33)]


def case_inputs(case, beta):
    key = ("inputs", case.id, beta)
    if key not in _cache:
        _cache[key] = _freeze(draws(stage(case.M, case.D, beta), case.n, case.M + case.D, case.zero_steps))
    return _cache[key]


def case_reference(case, beta):
    key = ("reference", case.id, beta)
    if key not in _cache:
        _cache[key] = _freeze(reference(stage(case.M, case.D, beta), case_inputs(case, beta)))
    return _cache[key]


# ---- Philox streams of plain and fixed-metric HMC ------------------------------------------------------------------------------------------
def philox_block(seed, chain_ids, it, block):
    """(U0, U1) of Philox4x32-10 blocks: counter (chain lo, chain hi, it, block), key seed; `block` broadcasts against chain_ids[:, None]"""
    g = np.asarray(chain_ids, dtype=np.uint64)[:, None]
    b = np.uint64(0) * g + np.asarray(block, dtype=np.uint64)
    g = g + np.uint64(0) * b
    key = (np.uint64(seed) & M32, np.uint64(seed) >> np.uint64(32))
    c = philox4x32_10((g & M32, g >> np.uint64(32), np.full_like(g, np.uint64(it)), b), key)
    return _u53(c[0], c[1]), _u53(c[2], c[3])


def hmc_streams(seed, chain_ids, D, it, with_radius=False):
    """(z [n][D], u_len [n], u_acc [n]) of transition `it` of the chains: z from blocks d / 2 by Box-Muller, cos for even d and sin for
    odd; (u_len, u_acc) = (U0, U1) of block 0x40000000.  with_radius: also sqrt(-2 ln U0) per element of z."""
    j = np.arange(D, dtype=np.uint64)[None, :]
    odd = (j & np.uint64(1)) == 1
    U0, U1 = philox_block(seed, chain_ids, it, j >> np.uint64(1))
    rad = np.sqrt(-2.0 * np.log(U0))
    z = rad * np.where(odd, np.sin(2 * np.pi * U1), np.cos(2 * np.pi * U1))
    u_len, u_acc = philox_block(seed, chain_ids, it, np.uint64(BLOCK_LEN_ACC))
    out = (z, u_len[:, 0], u_acc[:, 0])
    return out + (rad,) if with_radius else out


def sampler_ref(problem, theta0, T, L, eps, seed, chain_offset, beta=None, z_factor=1.0):
    """the restatement's transition chained over the iterations 0..T-1 of every chain on those streams (problem: a dict of `stage` or
    `identity_problem`).  Returns dict(samples [n][T][D] the state after each iteration, accepted, nsteps, status [n][T], margin: the
    smallest distance of a decision from a tie; with beta also loglik0 [n] at theta0 and loglik [n] at the last state).
    z_factor multiplies every z: the probe of tests/test_phmc_edges_cpu.py for decisions that hang on a rounding."""
    W = np.array(theta0, dtype=np.float64)
    n, D = W.shape
    ids = chain_offset + np.arange(n)
    out = dict(samples=np.empty((n, T, D)), accepted=np.zeros((n, T), dtype=np.int64), nsteps=np.zeros((n, T), dtype=np.int64),
               status=np.zeros((n, T), dtype=np.int64), margin=np.inf)
    for it in range(T):
        z, u_len, u_acc = hmc_streams(seed, ids, D, it)
        r = reference(dict(problem, beta=beta), dict(w=W, z=z * z_factor, u_len=u_len, u_acc=u_acc), L, eps)
        W = r["w"]
        out["samples"][:, it] = W
        for k in ("accepted", "nsteps", "status"):
            out[k][:, it] = r[k]
        with np.errstate(invalid="ignore"):
            out["margin"] = float(min(out["margin"], np.abs(r["margin"]).min()))
        if beta is not None:
            if it == 0:
                out["loglik0"] = r["loglik0"]
            out["loglik"] = r["loglik"]
    return out


# ---- sampler table -----------------------------------------------------------------------------------------------------------------------
# Only in a sampling run do the chains of a workgroup begin their transitions at different global steps: k_phmc_head then has begun
# chains (a column of z) and stepping chains (a zero column in Lm z, p0 read from ch.p) side by side, and chains reach iter_limit at
# different times.  33 chains at D = 17: two full workgroups and one chain; 18 chains at the NDB 4 | 8 | 12 | 16 edges.
SamplerCase = collections.namedtuple("SamplerCase", "id M D n beta why")
SAMPLER_T, SAMPLER_BURN_IN, SAMPLER_SEED, SAMPLER_OFFSET = 6, 2, 2 ** 40 + 31, 7
SAMPLER_SHAPES = [(300, 17, 33, (None,)), (300, 49, 18, (None, 0.3)), (300, 128, 18, (None,)), (300, 129, 18, (None, 0.3)),
                  (300, 255, 18, (None,))]
SAMPLER_CASES = [SamplerCase("s-%dx%dx%d%s" % (_M, _D, _n, "" if _b is None else "-beta%g" % _b), _M, _D, _n, _b,
                             "%s sampler, NDB %d, %d workgroup(s), last holds %d" % ("PHMC" if _b is None else "tempered", ndb_of(_D),
                                                                                    (_n + 15) // 16, _n - 16 * ((_n + 15) // 16 - 1)))
                 for _M, _D, _n, _bs in SAMPLER_SHAPES for _b in _bs]


def sampler_theta0(case):
    key = ("theta0", case.id)
    if key not in _cache:
        _cache[key] = _freeze(draws(stage(case.M, case.D, case.beta), case.n, case.M + case.D + case.n))["w"]
    return _cache[key]


def sampler_reference(case, seed=SAMPLER_SEED, z_factor=1.0):
    key = ("sampler", case.id, seed, z_factor)
    if key not in _cache:
        _cache[key] = _freeze(sampler_ref(stage(case.M, case.D, case.beta), sampler_theta0(case), SAMPLER_T, L, EPS, seed, SAMPLER_OFFSET,
                                          case.beta, z_factor))
    return _cache[key]


# ---- a failing chain among neighbours ------------------------------------------------------------------------------------------------------
# the header of csrc/phmc.hip.h: "a chain is a COLUMN of the product, so a chain that carries NaN or inf cannot reach its neighbours".
# Chain 5: slot jj = 1 of wavefront 1, with neighbours in the same wavefront and the same product; chain 17: the second workgroup.
PLANT_SHAPES = [(300, 129, 18), (300, 49, 18)]
PLANTED = (5, 17)
PLANT_KINDS = ("w_nan", "w_inf", "z_nan")


def plant_case(M, D, n, kind, beta):
    """(stage, planted inputs, twin inputs): the twin is the same batch with its benign draw in every planted entry (the recipe of
    failing_chains.hmc_case).  No zero-step chain: the planted chains step, so a NaN momentum meets the head's PHMC_NAN branch."""
    st = stage(M, D, beta)
    twin = draws(st, n, M + D + 1)
    planted = {k: v.copy() for k, v in twin.items()}
    for c in PLANTED:
        if kind == "w_nan":
            planted["w"][c, min(3, D - 1)] = np.nan
        elif kind == "w_inf":
            planted["w"][c, D - 1] = np.inf
        elif kind == "z_nan":
            planted["z"][c, D // 2] = np.nan
        else:
            raise ValueError(kind)
    return st, _freeze(planted), _freeze(twin)


# ---- the prior draws -------------------------------------------------------------------------------------------------------------------------
PRIOR_D = (1, 2, 63, 64, 65, 255)
PRIOR_N, PRIOR_SEED, PRIOR_OFFSET = 18, 2 ** 40 + 5, 9


def prior_reference(D, n=PRIOR_N, seed=PRIOR_SEED, chain_offset=PRIOR_OFFSET):
    """(sqrt(alpha) z, the bound per element) of rmhmc_ais_prior: z of hmc_streams at iteration counter 0xFFFFFFFF.  Bound:
    64 * 2^-53 * sqrt(alpha) * sqrt(-2 ln U0).  It covers the rounding of the angle 2 pi U1 < 6.3 on both sides, which moves sin and
    cos by about 13 x 2^-53 absolute (2 pi x 2^-53 per side), and a few ulp each for log, sqrt and sin / cos, relative to a factor that
    is at most 1 in size."""
    z, _, _, rad = hmc_streams(seed, chain_offset + np.arange(n), D, PRIOR_ITER, with_radius=True)
    return math.sqrt(ALPHA) * z, 64.0 * 2.0 ** -53 * math.sqrt(ALPHA) * rad
