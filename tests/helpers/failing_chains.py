"""Harness of tests/test_failing_chains_cpu.py and tests/test_gpu_failing_chains.py: batches in which some chains fail (a NaN or inf
position, a trajectory that overflows, a Cholesky pivot <= 0) or trip the reference's guards while their neighbours are well behaved.

The contract under test (include/rmhmc.h, next to the status bits): a chain that fails is rejected, keeps its state, carries at
least one failure bit, and does not change one bit of any other chain of its batch.  It is implemented once per stepping path
(fused, one-launch medium step, generic, int8, large-D), so every case runs on every path, with and without RMHMC_COMPAT.

GPU-free: shapes, plants and inputs only; the libraries are driven by the two test files."""
import numpy as np

from riemannhamiltonianmontecarlo_amd import _capi
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg
from context_history import PATHS
from plan_probe import plan

FAIL = _capi.ST_NOT_PD | _capi.ST_NONFINITE
GUARDS = _capi.ST_GUARD_P | _capi.ST_GUARD_W
MODES = {"plain": 0, "compat": _capi.COMPAT}

# chains per batch: M, D, the int8 bits and the data seed are those of context_history.PATHS, the batch is large enough for edges of
# the 16-chain wavefront groups (0 | 15 | 16) and, on the int8 path, of the 128-chain tiles (127 | 128)
N_CHAINS = {"fused": 40, "medium": 40, "generic": 40, "generic_rowsplit": 70, "int8": 130, "int8_s5": 40, "large": 20, "large_int8": 20}
L, EPS, K = 3, 0.4, 4                       # the transition of context_history's battery

KINDS = ("nan", "inf", "w60", "z300", "w3", "z20")
POISONED = ("nan", "inf")                   # non-finite in the input itself
MOMENTUM_GUARD = ("z300", "z20")            # |p| > 100 under RMHMC_FLAG_GUARDS: renormalised, the trajectory then stays finite
FAR_OUT = ("nan", "inf", "w60")             # the plants of the leapfrog isolation check (rmhmc_leapfrog draws no momentum)


def spec_of(path, mode, n=None):
    """(M, D, n, flags, data seed) of a path in a flag mode"""
    M, D, _, flags, seed = PATHS[path]
    return (M, D, N_CHAINS[path] if n is None else n, (flags & ~_capi.COMPAT) | MODES[mode], seed)


def data_of(spec):
    return synthetic_logreg(spec[0], spec[1], spec[4])


def context(lib, spec, options=None):
    """a context of `lib` for the shape with the path's data; the oracle gets the flags it knows (it is fp64 throughout)"""
    M, D, n, flags, _ = spec
    ctx = lib.context(M, D, n, flags=flags if lib.on_gpu else flags & _capi.COMPAT, options=options)
    ctx.set_data(*data_of(spec), 100.0)
    return ctx


def assert_shape_on_path(path, spec):
    """the planning rule itself (csrc/plan.h through the probe) still sends the shape to the path it was chosen for"""
    M, D, n, flags, _ = spec
    p = plan(M, D, n, flags)
    want = {"fused": (1, 0, 0), "medium": (0, 1, 0), "large": (0, 0, 1), "large_int8": (0, 0, 1)}.get(path, (0, 0, 0))
    assert (p["fused"], p["medium"], p["big"]) == want, (path, p)
    assert bool(p["i8_requested"]) == bool(flags & _capi.FLAG_INT8_METRIC), (path, p)
    if path == "generic":
        assert p["fsplit"] == 1, p
    if path == "generic_rowsplit":
        assert p["fsplit"] > 1, p
    if path == "large_int8":
        assert p["gbase"], p


def plant_positions(n):
    """0 | 15 | 16 and the last chain, 127 | 128 where the batch has them, filled up to one position per kind.  The fill never plants
    more than half of a 16-chain group (the required positions do only in a ragged last group of two)."""
    pos = [0, 15, 16, n - 1] + ([127, 128] if n > 128 else [])
    pos = sorted(set(p for p in pos if 0 <= p < n))
    for cand in range(5, n, 4):
        if len(pos) >= len(KINDS):
            break
        group = [p for p in pos if p // 16 == cand // 16]
        size = min(16, n - 16 * (cand // 16))
        if cand not in pos and 2 * (len(group) + 1) <= size:
            pos.append(cand)
    assert len(pos) >= len(KINDS), (n, pos)
    return sorted(pos)


def plants_of(path):
    """[(chain, kind)]: the kinds rotate with the path, so that over the table every kind meets every kind of edge"""
    pos = plant_positions(N_CHAINS[path])
    shift = list(PATHS).index(path)
    return [(p, KINDS[(i + shift) % len(KINDS)]) for i, p in enumerate(pos)]


def base_inputs(spec):
    """benign arguments of rmhmc_transition, drawn like context_history.make_inputs"""
    M, D, n, _, seed = spec
    rs = np.random.RandomState(2000 + seed)
    return dict(w=0.2 * rs.randn(n, D) / np.sqrt(D), z=rs.randn(n, D), ul=rs.rand(n), gd=rs.randn(n), ua=rs.rand(n))


def apply_plant(w, z, chain, kind):
    D = w.shape[1]
    if kind == "nan":
        w[chain, min(3, D - 1)] = np.nan
    elif kind == "inf":
        w[chain, D - 1] = np.inf
    elif kind == "w60":
        w[chain] = 60.0
    elif kind == "w3":
        w[chain] = 3.0
    elif kind == "z300":
        z[chain] *= 300.0
    elif kind == "z20":
        z[chain] *= 20.0
    else:
        raise ValueError(kind)


def make_case(path, mode, kinds=KINDS):
    """(spec, planted inputs, twin inputs, [(chain, kind)]): the twin is the same batch with a benign draw in every planted row"""
    spec = spec_of(path, mode)
    twin = base_inputs(spec)
    planted = {k: v.copy() for k, v in twin.items()}
    plants = [(c, kind) for c, kind in plants_of(path) if kind in kinds]
    for c, kind in plants:
        apply_plant(planted["w"], planted["z"], c, kind)
    for d in (twin, planted):
        for v in d.values():
            v.setflags(write=False)
    return spec, planted, twin, plants


def transition(ctx, inp):
    with np.errstate(all="ignore"):
        return ctx.transition(inp["w"], inp["z"], inp["ul"], inp["gd"], inp["ua"], L=L, eps=EPS, K=K)


_oracle_cache = {}


def oracle_transition(oracle, path, mode):
    """the planted batch on the oracle, once per process, read-only"""
    key = (path, mode)
    if key not in _oracle_cache:
        spec, planted, _, _ = make_case(path, mode)
        with context(oracle, spec) as ctx:
            r = transition(ctx, planted)
        for v in r.values():
            v.setflags(write=False)
        _oracle_cache[key] = r
    return _oracle_cache[key]


# ---- samplers that fail and carry on -----------------------------------------------------------------------------------------------
# path -> (flag mode, step size, chains).  Step sizes so large that many trajectories overflow or lose positive definiteness while the
# chains still move: tests/test_failing_chains_cpu.py checks on the oracle that every row really is in that regime.
SAMPLER_CASES = {
    "fused": ("plain", 1.6, 48),
    "medium": ("compat", 1.4, 48),
    "generic": ("plain", 1.0, 48),
    "generic_rowsplit": ("compat", 1.0, 48),
    "int8": ("plain", 1.0, 130),
    "int8_s5": ("plain", 1.0, 48),
    "large": ("plain", 0.5, 20),
    "large_int8": ("compat", 0.6, 20),
}
SAMPLER_T, SAMPLER_L, SAMPLER_K, SAMPLER_SEED = 16, 4, 4, 77
REGIME_N, REGIME_ITERS = 48, 20


def sampler_spec(path):
    mode, eps, n = SAMPLER_CASES[path]
    return spec_of(path, mode, n), eps


def sampler_theta0(spec):
    M, D, n, _, seed = spec
    return 0.01 * np.random.RandomState(3000 + seed).randn(n, D)


def sample(ctx, eps, theta0):
    with np.errstate(all="ignore"):
        s, acc, steps, _ = ctx.sample(SAMPLER_T, 0, L=SAMPLER_L, eps=eps, K=SAMPLER_K, seed=SAMPLER_SEED, theta0=theta0)
    return {"samples": s, "accepted": acc, "leapfrog_steps": steps}


# ---- plain HMC and mMALA -----------------------------------------------------------------------------------------------------------
# the stepping paths of rmhmc_hmc_transition that test_hmc_sampler_matches_oracle_and_shim (400, 12, 2) does not reach
HMC_SHAPES = {
    "generic": (300, 40, 40, 33, 0.005),
    "large": (200, 70, 20, 37, 0.005),
    "traj_rows_in_registers": (270, 14, 40, 32, 0.005),
    "traj_rows_streamed": (3000, 30, 8, 41, 0.001),
}
# (M, D, n, data seed, step size: the planted chain's momentum is NaN after its first gradient whatever the step size; the existing
#  check's 0.5 makes every chain of these larger shapes overflow on data x 50, so each shape has a step size at which the neighbours
#  stay finite and some of them accept)
HMC_X_SCALE, HMC_FAR, HMC_L = 50.0, 300.0, 10
MMALA_SHAPES = {"medium": PATHS["medium"], "generic": PATHS["generic"], "large": PATHS["large"]}
MMALA_N = {"medium": 40, "generic": 40, "large": 20}


def hmc_case(name):
    """(M, D, n, XX, t, planted inputs, twin inputs, planted chain, step size): the recipe of the existing check, data x 50 and one chain at
    w = 300, whose first gradient overflows the momentum"""
    M, D, n, seed, eps = HMC_SHAPES[name]
    XX, t = synthetic_logreg(M, D, seed)
    rs = np.random.RandomState(4000 + seed)
    twin = dict(w=0.01 * rs.randn(n, D), z=rs.randn(n, D), ul=rs.rand(n), ua=rs.rand(n))
    c = 17 if n > 17 else n - 2
    planted = {k: v.copy() for k, v in twin.items()}
    planted["w"][c] = HMC_FAR
    return M, D, n, XX * HMC_X_SCALE, t, planted, twin, c, eps


def hmc_transition(ctx, inp, eps):
    with np.errstate(all="ignore"):
        return ctx.hmc_transition(inp["w"], inp["z"], inp["ul"], inp["ua"], L=HMC_L, eps=eps)


def mmala_case(name):
    M, D, _, _, seed = MMALA_SHAPES[name]
    n = MMALA_N[name]
    rs = np.random.RandomState(5000 + seed)
    twin = dict(w=0.1 * rs.randn(n, D), z=rs.randn(n, D), ua=rs.rand(n))
    c = 16 if n > 17 else n - 2
    planted = {k: v.copy() for k, v in twin.items()}
    planted["w"][c, min(3, D - 1)] = np.nan
    return (M, D, n, 0, seed), planted, twin, c


def mmala_transition(ctx, inp):
    with np.errstate(all="ignore"):
        return ctx.mmala_transition(inp["w"], inp["z"], inp["ua"], 0.5)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and (np.array_equal(a, b, equal_nan=True) if a.dtype.kind == "f" else np.array_equal(a, b))
