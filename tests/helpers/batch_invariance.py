"""Harness of tests/test_batch_invariance_cpu.py and tests/test_gpu_batch_invariance.py: a chain's output is a function of (data, seed,
global chain id, run arguments) and of the plan of its context - not of how many chains share the context, of the slot it occupies or
of its neighbours.  DESIGN section 7 and multi_gpu.py rest on that.

One case per stepping path, each at the smallest chain count that crosses the path's chain-count edges (16-chain wavefront groups,
64-chain momentum grids, 128-chain int8 tiles), every one at M = 300 on `synthetic_logreg`.  Every context gets the create options
OPTIONS, under which the plan of a shape (csrc/plan.h) does not move with the chain count: `signature` is what is left of the probe's
answer once the chain count and the sizes padded from it are taken out, and tests/test_batch_invariance_cpu.py shows that it is the same
for the whole batch and every sub-batch.  With the default options it is not (row splits and the stepping path follow the chain count):
THRESHOLDS lists the shapes at which the default plans part, which is the condition DESIGN section 7 states.

A case is run once as a whole batch and once per sub-batch: a contiguous range [a, b) of its chains in a context of b - a chains, whose
inputs are the rows [a, b) of the whole batch's (`take`), its `chain_offset` BASE + a and its `theta0` the rows [a, b).  The ranges
move every chain but the first to another slot, wavefront group and tile and hit the remainders; PERM moves every chain for the calls
that take their random numbers as arguments.  Inputs, battery and step sizes are those of tests/helpers/shape_edges.py.

GPU-free: the libraries are driven by the two test files."""
import numpy as np

import shape_edges as E
from plan_probe import probe_line, probe_many
from riemannhamiltonianmontecarlo_amd import _capi

I8 = _capi.int8_metric_flags
M = 300
OPTIONS = {"nsplit_max": 4, "fsplit": 1}
BASE = 3                        # chain_offset of the whole batch: a sub-batch [a, b) runs at BASE + a
SEED = 77
N_ITER, BURN_IN = 12, 4
CHAIN_COUNTS = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 130, 257)    # the signature holds still over all of these


def _case(name, D, n, why, flags=0, options=None, calls="all"):
    c = E._case("batch", M, D, n, why, flags=flags, options=dict(OPTIONS, **(options or {})))
    return c._replace(id=name), calls


_TABLE = [
    _case("fused", 5, 9, "k_fused_small: one wavefront per chain, four chains per workgroup"),
    _case("medium_nb1", 12, 19, "k_step_medium<1, .>: a workgroup per chain"),
    _case("medium_nb2", 20, 19, "k_step_medium<2, .>"),
    _case("generic_nb2", 20, 81, "generic fp64 kernels at NB = 2 (medium = 0 turns k_hmc_traj off as well)", options=E.NO_MEDIUM),
    _case("generic", 40, 81, "generic fp64 kernels: 81 = 64 + 16 + 1 chains"),
    _case("hmc_traj", 20, 81, "k_hmc_traj: plain HMC, one launch per trajectory", calls="hmc"),
    _case("i8s6", 40, 130, "int8 assembly, 6 slices: 130 = 128 + 2 chains, per-chain v exponent, delta assemblies", flags=I8(6)),
    _case("i8s5", 40, 130, "int8 assembly, 5 slices (Z fragments from global memory)", flags=I8(5)),
    _case("i8s7", 40, 130, "int8 assembly, 7 slices: the 64-pair tile", flags=I8(7)),
    _case("i8s4", 40, 130, "int8 assembly, 4 slices (Z fragments from global memory)", flags=I8(4)),
    _case("large", 70, 18, "blocked large-D path, two column blocks"),
    _case("large_i8", 70, 130, "blocked large-D path with the int8 assembly (copy of G for the delta assemblies)", flags=I8(6)),
    _case("compat", 40, 81, "generic fp64 kernels with the reference's guards", flags=_capi.COMPAT),
]
CASES = [c for c, _ in _TABLE]
CALLS = {c.id: calls for c, calls in _TABLE}
BY_ID = {c.id: c for c in CASES}
IDS = [c.id for c in CASES]
assert len(BY_ID) == len(CASES)

# the path each case is for: (fused, medium, big, hmc_traj, int8 slices) of its plan
PATHS = {"fused": (1, 0, 0, 1, 0), "medium_nb1": (0, 1, 0, 1, 0), "medium_nb2": (0, 1, 0, 1, 0), "generic_nb2": (0, 0, 0, 0, 0),
         "generic": (0, 0, 0, 0, 0), "hmc_traj": (0, 1, 0, 1, 0), "i8s6": (0, 0, 0, 0, 6), "i8s5": (0, 0, 0, 0, 5), "i8s7": (0, 0, 0, 0, 7),
         "i8s4": (0, 0, 0, 0, 4), "large": (0, 0, 1, 0, 0), "large_i8": (0, 0, 1, 0, 6), "compat": (0, 0, 0, 0, 0)}

_RANGES = {
    81: [(0, 16), (15, 16), (16, 33), (64, 81), (1, 66)],
    130: [(0, 128), (127, 130), (64, 65), (1, 130)],
}


def ranges(case):
    """the sub-batches [a, b) of a case"""
    n = case.n
    if n in _RANGES:
        return list(_RANGES[n])
    assert n in (9, 18, 19), n
    return [(n // 2, n // 2 + 1), (1, n), (n - 1, n)]      # a single chain, a range that starts at slot 1, the last chain alone


def perm(case):
    """one fixed permutation of the whole batch that leaves no chain in its slot"""
    n = case.n
    r = np.random.RandomState(n).permutation(n)
    p = np.empty(n, dtype=np.int64)
    p[r] = np.roll(r, -1)                                  # one cycle through the chains in a random order
    assert sorted(p.tolist()) == list(range(n)) and not (p == np.arange(n)).any()
    return p


def sub(case, n):
    """the case at another chain count"""
    return case._replace(n=int(n))


def take(x, rows):
    """rows of every per-chain array of a dict of inputs or outputs: `rows` a (a, b) range or an index array"""
    idx = slice(*rows) if isinstance(rows, tuple) else np.asarray(rows)
    return {k: np.array(v[idx], order="C") for k, v in x.items()}       # (copies: a row range of a contiguous array would be a view)


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
_NOT_IN_SIGNATURE = ("n", "nCp")       # the chain count and what is padded from it


def _signature_of(r):
    assert r["check"]["code"] == 0 and r["option_error"] is None, r
    sig = {k: v for k, v in r["plan"].items() if k not in _NOT_IN_SIGNATURE}
    sig["amh"] = (r["amh"]["nt"], r["amh"]["rows"])
    if "i8" in r:      # the tile shape, whether the ragged pair block runs as tiles of its own, and the k pieces of one assembly
        sig["i8"] = (r["i8"]["WN"], r["i8"]["TN"], r["i8"]["tail"], r["i8"]["nPB"], r["i8"]["npb"],
                     tuple((k["ks0"], k["nk"], k["tail_pieces"]) for k in r["i8"]["k_pieces"]))
    return sig


def signatures(case, counts):
    """signature(case, n) for every n of `counts`, from one run of the probe"""
    rs = probe_many([probe_line(case.M, case.D, n, case.flags, options=case.options) for n in counts])
    return [_signature_of(r) for r in rs]


def signature(case, n=None):
    """what csrc/plan.h decides for the case's shape and options at n chains, without the chain count and the sizes padded from it:
    every field of Plan but n and nCp, amh_shape, and the int8 launch geometry that does not scale with the batch"""
    return signatures(case, [case.n if n is None else n])[0]


def sig_diff(a, b):
    """the fields in which two signatures differ: {field: (a's, b's)}"""
    return {k: (a.get(k), b.get(k)) for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)}


def sig_text(case):
    s = signature(case)
    path = "fused" if s["fused"] else "medium" if s["medium"] else "large" if s["big"] else "generic"
    t = "%s NB %d Mp %d nsplit %d fsplit %d hmc_traj %d amh %s" % (path, s["NB"], s["Mp"], s["nsplit"], s["fsplit"], s["hmc_traj"], s["amh"])
    if s["i8_requested"]:
        t += " i8S %d bn %d nks %d NP %d ksplit %d/%d tail_acc %d tail_pieces %d gbase %d lev_full %d" % (
            s["i8S"], s["i8_bn"], s["i8_nks"], s["NP"], s["ksplit_a"], s["ksplit_l"], s["tail_acc"], s["tail_pieces"], s["gbase"], s["i8_lev_full"])
    return t


def check_path(case):
    """the case is planned onto the path it is named for"""
    s = signature(case)
    got = (s["fused"], s["medium"], s["big"], s["hmc_traj"], s["i8S"] if s["i8_requested"] else 0)
    assert got == PATHS[case.id], (case.id, got, s)
    assert s["nsplit"] == 4 and s["fsplit"] == 1, (case.id, s)
    return s


# Where the DEFAULT plans of a job and of its shards part (no create options): job (M, D, n, flags), shard chain count, the fields
# that must differ and those (of the ones sharding could move) that must not.  auto: flags from _capi.auto_metric_flags per context.
THRESHOLDS = [
    dict(id="medium_at_512", M=1000, D=20, n=600, shard=300, differ={"medium": (0, 1), "nsplit": (54, 64)}, same=("hmc_traj",)),
    dict(id="fsplit_below_1024", M=1000, D=40, n=1040, shard=520, differ={"fsplit": (1, 4), "nsplit": (32, 63)}, same=("medium", "hmc_traj")),
    dict(id="hmc_traj_long_data", M=2000, D=20, n=600, shard=300, differ={"medium": (0, 1), "hmc_traj": (0, 1), "fsplit": (4, 7)}, same=()),
    dict(id="auto_int8", M=1000, D=40, n=700, shard=350, auto=True, differ={"i8_requested": (1, 0), "i8S": (6, 0)}, same=("medium",)),
]
# the smallest shapes at which the default plans part, which the GPU test runs: (M, D, whole, shard, fields that differ)
GPU_THRESHOLDS = {
    "medium": (300, 20, 514, 257, {"medium": (0, 1)}),
    "fsplit": (600, 40, 1100, 550, {"fsplit": (1, 2)}),
}
AMH_THRESHOLD = (300, 1024, 512)       # amh_shape(M, n): one wavefront per chain from 1024 chains, a 256-thread workgroup below


def default_plans(M_, D, n, shard, auto=False):
    """the default-option plans of a job of n chains and of a shard of `shard` chains"""
    fl = [_capi.auto_metric_flags(D, k, M=M_) & ~_capi.FLAG_INT8_CERTIFY if auto else 0 for k in (n, shard)]
    rs = probe_many([probe_line(M_, D, k, f) for k, f in zip((n, shard), fl)])
    for r in rs:
        assert r["check"]["code"] == 0, r
    return rs


# ---- contexts, inputs and calls ---------------------------------------------------------------------------------------------------------
def context(lib, case):
    return E.context(lib, case)


def inputs(case, oracle):
    """the inputs of the whole batch: those of shape_edges (momentum from the oracle's Cholesky factor)"""
    return E.inputs(case, oracle)


def battery(ctx, i, case):
    """shape_edges' battery; the hmc_traj case runs the plain-HMC call alone"""
    if CALLS[case.id] == "hmc":
        with np.errstate(all="ignore"):
            return {"hmc." + k: v for k, v in ctx.hmc_transition(i["w"], i["z"], i["u_len"], i["u_acc"], L=E.HMC_L, eps=E.HMC_EPS).items()}
    return E.battery(ctx, i, case)


def samplers_of(case, lib):
    """the samplers a case runs on a library: the oracle has the first three; IWLS and Gibbs stop at D = 64"""
    if CALLS[case.id] == "hmc":
        return ["hmc_sample"]
    s = ["sample", "hmc_sample", "mmala_sample"]
    if lib.on_gpu:
        s += ["amh"] + (["iwls", "gibbs"] if case.D <= 64 else [])
    return s


def run_sampler(ctx, name, case, theta0, a=0):
    """one sampler on a context that holds the chains [a, a + ctx.n) of the whole batch: {output: array}, samples and every counter"""
    kw = dict(seed=SEED, chain_offset=BASE + a)
    with np.errstate(all="ignore"):
        if name == "sample":
            s, acc, steps, _ = ctx.sample(N_ITER, BURN_IN, E.L, case.eps, E.K, theta0=theta0, **kw)
            return {"samples": s, "accepted": acc, "leapfrog_steps": steps}
        if name == "hmc_sample":
            s, acc, steps, _ = ctx.hmc_sample(N_ITER, BURN_IN, E.HMC_L, E.HMC_EPS, theta0=theta0, **kw)
            return {"samples": s, "accepted": acc, "leapfrog_steps": steps}
        if name == "mmala_sample":
            s, acc, _ = ctx.mmala_sample(N_ITER, BURN_IN, E.MMALA_EPS, theta0=theta0, **kw)
            return {"samples": s, "accepted": acc}
        if name == "gibbs":                                                  # (no theta0: include/rmhmc_gibbs.h)
            r = ctx.sample_to("gibbs", N_ITER, BURN_IN, samples=True, **kw)
        else:
            r = ctx.sample_to(name, N_ITER, BURN_IN, samples=True, theta0=theta0, **kw)
    r.pop("seconds")
    return r


def run_chains(ctx, case, theta0, a=0, steps=(3, 4)):
    """the timed path: chains_init, two chains_run calls, chains_state"""
    with np.errstate(all="ignore"):
        ctx.chains_init(theta0=theta0, seed=SEED, chain_offset=BASE + a, L=E.L, eps=case.eps, K=E.K)
        for k in steps:
            ctx.chains_run(k)
        w, it, acc = ctx.chains_state()
    return {"w": w, "iters": it, "accepted": acc}


# ---- the comparator ---------------------------------------------------------------------------------------------------------------------
def bits_differ(whole, part, rows):
    """The outputs of a sub-batch against the rows of the whole batch's, bit for bit (`tobytes`: NaN payloads and signed zeros count).
    Returns one line per output that differs, [] when all are equal.  `rows`: the (a, b) range or the index array the sub-batch holds."""
    idx = slice(*rows) if isinstance(rows, tuple) else np.asarray(rows)
    bad = []
    assert set(whole) == set(part), (sorted(whole), sorted(part))
    for k in sorted(whole):
        w, p = np.ascontiguousarray(np.asarray(whole[k])[idx]), np.ascontiguousarray(part[k])
        if w.dtype != p.dtype or w.shape != p.shape:
            bad.append("%s: %s%s against %s%s" % (k, w.dtype, w.shape, p.dtype, p.shape))
        elif w.tobytes() != p.tobytes():
            ne = (w.view(np.uint8).reshape(len(w), -1) != p.view(np.uint8).reshape(len(p), -1)).any(axis=1) if len(w) else np.zeros(0, bool)
            first = int(np.nonzero(ne)[0][0])
            d = ""
            if w.dtype.kind == "f":
                with np.errstate(all="ignore"):
                    d = ", largest difference %.3e" % float(np.nanmax(np.abs(w.astype(np.float64) - p)))
            bad.append("%s: %d of %d chains differ, first at row %d of the sub-batch%s" % (k, int(ne.sum()), len(w), first, d))
    return bad


def delta_batch(case, oracle, scale):
    """The inputs of the delta-slice test: every chain takes two leapfrog steps, and chain 0's momentum is `scale` times the others'
    scale, so that its position iterates - and with them max |N_new - N_old| of the launch, from which the delta assemblies pick their
    slice count - move much further than the rest."""
    i = dict(inputs(case, oracle))
    p = i["p"].copy()
    p[0] *= scale
    i["p"] = p
    i["ns"] = np.full(case.n, 2, dtype=np.int32)
    return i


def delta_leapfrog(ctx, i, case):
    with np.errstate(all="ignore"):
        w, p, hld, st = ctx.leapfrog(i["w"], i["p"], case.eps, i["dr"], i["ns"], E.K)
    return {"w": w, "p": p, "hld": hld, "status": st}


DELTA_SCALE = {"i8s6": 6.0, "large_i8": 6.0}
DELTA_RANGES = [(1, 130), (1, 65)]          # sub-batches without chain 0
