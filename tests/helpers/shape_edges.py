"""Harness of tests/test_shape_edges_cpu.py and tests/test_gpu_shape_edges.py: the RMHMC core at the tile, block and padding edges of
every stepping path (fused_small, medium_step, the generic fp64 kernels, the int8 metric, the blocked large-D path).

Each path is templated or blocked on the shape: NB = ceil(D / 16) column tiles, 64-column blocks above D = 64, rows padded to Mp (64),
16-chain wavefront groups, 64-chain grids of the momentum passes, 128-chain int8 tiles, 32-row int8 k-stages, 128- and 32-pair blocks of
the lower triangle, rows per thread of the one-launch step.  The tables below hold one small shape per edge; `why` says which kernel
variant or remainder the case is there for, and `edges()` derives the figures (NB and ragged columns, blocks, k-stages, pair-block rest,
chain-group rest) from the plan of the shape itself.

GPU-free: shapes, inputs, the battery of calls and the plan each case must get.  The libraries are driven by the two test files.  The
battery of a case is computed once per process on the oracle, shared and read-only."""
import collections

import numpy as np

from riemannhamiltonianmontecarlo_amd import _capi
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg
from plan_probe import plan

I8 = _capi.int8_metric_flags
DATA_SEED, ALPHA = 17, 100.0
EPS, L, K = 0.1, 3, 4          # RMHMC.  (At eps 0.2 the M < D = 70 cases overflow in the oracle, at 0.5 most small-M cases do.
#                                The int8 row-count cases M = 31, 32, 33 stay finite at 0.1 as well: test_shape_edges_cpu.py.)
HMC_L, HMC_EPS = 8, 0.02
MMALA_EPS = 0.1

# path: "fused" | "medium" | "generic" | "large", the stepping path the plan must choose (csrc/plan.h); the int8 metric is a flag on top
Case = collections.namedtuple("Case", "id table M D n flags options path eps why")


def slices(case):
    """byte slices of the int8 metric, 0 on the fp64 matrix cores"""
    return (case.flags >> 12) & 7 if case.flags & _capi.FLAG_INT8_METRIC else 0


def _path_of(D, options):
    if D > 64:
        return "large"
    if D <= 8:
        return "fused"
    return "medium" if D <= 32 and options.get("medium", 1) else "generic"


def _case(table, M, D, n, why, flags=0, options=None, eps=EPS):
    options = dict(options or {})
    S = (flags >> 12) & 7 if flags & _capi.FLAG_INT8_METRIC else 0
    path = _path_of(D, options)
    name = "%s-%dx%dx%d-%s%s%s" % (table, M, D, n, path, "-i8s%d" % S if S else "", "-compat" if flags & _capi.COMPAT else "")
    return Case(name, table, M, D, n, flags, options, path, eps, why)


def _d_why(D):
    NB, r = (D + 15) // 16, D % 16
    return "NB = %d, %s" % (NB, "exact tiles" if r == 0 else "last tile holds %d of 16 columns" % r)


NO_MEDIUM = {"medium": 0}

# ---- D edges: (300, D, 18).  18 chains: one full 16-chain wavefront group and a group of two -------------------------------------------
D_EDGES = (9, 16, 17, 31, 32, 47, 49, 63)
D_TABLE = []
for _D in D_EDGES:
    # generic fp64 kernels (k_rowpass / k_assemble / k_mompass / k_leverage / k_factor_full<NB>); D <= 32 would plan the one-launch step
    D_TABLE.append(_case("d", 300, _D, 18, "generic fp64, " + _d_why(_D), options=NO_MEDIUM if _D <= 32 else None))
for _D in D_EDGES:
    if _D <= 32:
        D_TABLE.append(_case("d", 300, _D, 18, "k_step_medium, " + _d_why(_D)))
for _D in D_EDGES:
    # int8 S = 6: the 8-wave tile (i8_bn 128, WN 4) and the pair layout; NP = D (D + 1) / 2 pairs, the rest after the 128-pair blocks
    D_TABLE.append(_case("d", 300, _D, 18, "int8 pair layout, %s, %d pairs = %d blocks of 128 + %d" % (_d_why(_D), _D * (_D + 1) // 2,
                         _D * (_D + 1) // 2 // 128, _D * (_D + 1) // 2 % 128), flags=I8(6), options=NO_MEDIUM))
for _D in (49, 63):
    for _S in (4, 5, 7):
        # S = 4, 5: the tiles that read Z from global memory (i8_zdirect); S = 7: the other tile shape, i8_bn = 64, WN = 2
        D_TABLE.append(_case("d", 300, _D, 18, "int8 %d slices (%s), %s" % (_S, "i8_bn 64, WN 2" if _S == 7 else "i8_bn 128, WN 4", _d_why(_D)),
                             flags=I8(_S)))

# ---- large-D block edges: (300, D, 3); 64-column blocks, 128-pair blocks of the int8 layout ------------------------------------------
LARGE_EDGES = (127, 128, 129, 191, 193, 255)
LARGE_TABLE = []
for _D in LARGE_EDGES:
    _nbk, _NP = (_D + 63) // 64, _D * (_D + 1) // 2
    _w = "%d blocks of 64 columns, last holds %d; %d pairs, rest %d after the 128-pair blocks" % (_nbk, _D - 64 * (_nbk - 1), _NP, _NP % 128)
    LARGE_TABLE.append(_case("large", 300, _D, 3, "large-D fp64, " + _w))
    LARGE_TABLE.append(_case("large", 300, _D, 3, "large-D int8, " + _w, flags=I8(6)))

# ---- row-count edges: (M, D, 5).  M <= 17: Mp = 64 = 4 units of 16 rows, which nsplit is clamped to; 63 / 65: around Mp ------------------
M_EDGES = (1, 15, 16, 17, 63, 65)
M_TABLE = []
for _M in M_EDGES:
    _w = "M = %d, Mp = %d: %d padded rows" % (_M, (_M + 63) // 64 * 64, (_M + 63) // 64 * 64 - _M)
    M_TABLE.append(_case("m", _M, 5, 5, "k_fused_small, " + _w))
    M_TABLE.append(_case("m", _M, 12, 5, "k_step_medium<1,1>, " + _w))
    M_TABLE.append(_case("m", _M, 12, 5, "generic fp64 NB 1, " + _w, options=NO_MEDIUM))
    M_TABLE.append(_case("m", _M, 40, 5, "generic fp64 NB 3 (M < D: prior-dominated metric), " + _w))
    M_TABLE.append(_case("m", _M, 70, 5, "large-D fp64, two blocks, " + _w))

# ---- int8 row-count edges: 32-row k-stages ------------------------------------------------------------------------------------------------
I8_M_EDGES = (1, 31, 32, 33)
I8_M_TABLE = []
for _M in I8_M_EDGES:
    _w = "M = %d: %d k-stage(s) of 32, last holds %d rows" % (_M, (_M + 31) // 32, _M - 32 * ((_M + 31) // 32 - 1))
    I8_M_TABLE.append(_case("i8m", _M, 40, 5, "int8 generic, " + _w, flags=I8(6)))
    I8_M_TABLE.append(_case("i8m", _M, 70, 5, "int8 large-D, " + _w, flags=I8(6)))

# ---- chain-count edges on the generic paths: (100, 40, n) as the whole batch -------------------------------------------------------------
N_TABLE = [_case("n", 100, 40, _n, "generic fp64, %d chains: %d wavefront group(s) of 16, last holds %d; %d mompass block(s) of 64"
                 % (_n, (_n + 15) // 16, _n - 16 * ((_n + 15) // 16 - 1), (_n + 63) // 64)) for _n in (1, 16, 17, 64, 65)]
N_TABLE += [_case("n", 100, 40, _n, "int8, %d chains: %d tile(s) of 128, last holds %d; %d wavefront group(s) of 16, last holds %d"
                  % (_n, (_n + 127) // 128, _n - 128 * ((_n + 127) // 128 - 1), (_n + 15) // 16, _n - 16 * ((_n + 15) // 16 - 1)), flags=I8(6))
            for _n in (1, 16, 17, 127, 128)]


# ---- variants of the one-launch step ------------------------------------------------------------------------------------------------------
def medium_variant(M, D):
    """(NB, R) of k_step_medium<NB, R> for a shape, the rule of launch_step_medium_nb (csrc/rmhmc_hip.hip): rpt = ceil(Mp / 256) rows per
    thread stay in registers (R = rpt) while rpt * 16 NB <= 64 doubles hold them, else they are streamed (R = 0)"""
    NB = (D + 15) // 16
    assert NB in (1, 2), D
    Mp = (M + 63) // 64 * 64
    rpt = (Mp + 255) // 256
    return NB, (rpt if rpt * 16 * NB <= 64 else 0)


# (M, D, n) -> the instantiation the case is there for; existing shapes reach <1,1>, <1,2>, <1,3> and <2,0>
MEDIUM_VARIANTS = {(1000, 12, 3): (1, 4), (1500, 16, 3): (1, 0), (200, 17, 3): (2, 1), (300, 31, 18): (2, 2)}
VARIANT_TABLE = [_case("variant", _M, _D, _n, "k_step_medium<%d,%d>" % MEDIUM_VARIANTS[(_M, _D, _n)])
                 for (_M, _D, _n) in MEDIUM_VARIANTS if (_M, _D, _n) != (300, 31, 18)]   # ((300, 31, 18) runs in the D table)

# ---- the reference's guards (RMHMC_COMPAT) at a ragged tile and at a block edge: the guards may fire, the status bits are the oracle's --
COMPAT_TABLE = [_case("compat", 300, 49, 18, "generic fp64 with guards, " + _d_why(49), flags=_capi.COMPAT),
                _case("compat", 300, 193, 3, "large-D fp64 with guards, 4 blocks, last holds 1 column", flags=_capi.COMPAT)]

# ---- the leverage GEMM from 5 of 6 slices at the large-D edges ---------------------------------------------------------------------------
# The library sums the int8 leverages x_n' G^-1 x_n from the 5 most significant of 6 slices, except below 4 rows per column
# (Plan::i8_lev_full, a heuristic on the shape: csrc/plan.h).  The issue fixes M = 300 for the large-D table, M = 100 for the chain
# counts and the shapes of the full-mMALA cases, all below 4 D: every int8 case of those tables runs the 6-slice leverage GEMM, and only
# the D table ((300, D <= 63, 18)) runs the 5-slice one that shapes with M >= 4 D use.  The cases below, M = 5 D, add the 5-slice
# instantiation at the large-D pair-block edges (three blocks with one column in the last; D = 255, no ragged pair block) and, among
# the full-mMALA cases, on both int8 branches of mode 2.
LEV5_TABLE = [_case("lev5", 5 * _D, _D, 3, "large-D int8, leverages from 5 slices, %d column blocks, pair rest %d" % ((_D + 63) // 64, _D * (_D + 1) // 2 % 128),
                    flags=I8(6)) for _D in (129, 255)]

TABLES = {"d": D_TABLE, "large": LARGE_TABLE, "m": M_TABLE, "i8m": I8_M_TABLE, "n": N_TABLE, "variant": VARIANT_TABLE, "compat": COMPAT_TABLE,
          "lev5": LEV5_TABLE}
CASES = [c for tab in TABLES.values() for c in tab]
assert len(set(c.id for c in CASES)) == len(CASES)

# ---- full mMALA (RMHMC_FLAG_MMALA_FULL: mode 2 of eval_point_phases, the trace term alone) on every leverage branch -------------------------
# The planning rule gives (300, 49, 18) one row range (Mp = 320 < 2 x 256), so the case runs twice: as planned, and with the create
# option fsplit = 4 (row ranges of 3, 3, 3 and 1 groups of 32 rows), which is the k_leverage / k_reduce_tr branch with partial planes.
FULL = _capi.FLAG_MMALA_FULL
MMALA_FULL_CASES = [
    _case("full", 300, 49, 18, "k_leverage<4>, one row range", flags=FULL, options=NO_MEDIUM),
    _case("full", 300, 49, 18, "k_leverage<4> in 4 row ranges + k_reduce_tr", flags=FULL, options={"medium": 0, "fsplit": 4})._replace(
        id="full-300x49x18-generic-fsplit4"),
    _case("full", 100, 40, 128, "generic int8: leverage GEMM + k_trvec<3>", flags=FULL | I8(6)),
    _case("full", 300, 129, 3, "k_leverage_pair / k_trace_big, 3 blocks", flags=FULL),
    _case("full", 300, 193, 3, "large-D int8: leverage GEMM + k_trace_big, 4 blocks", flags=FULL | I8(6)),
    # (the two int8 shapes above are below 4 D: 6-slice leverages.  M = 5 D: the 5-slice leverage GEMM on the same two branches)
    _case("full", 200, 40, 128, "generic int8: 5-slice leverage GEMM + k_trvec<3>", flags=FULL | I8(6)),
    _case("full", 965, 193, 3, "large-D int8: 5-slice leverage GEMM + k_trace_big, 4 blocks", flags=FULL | I8(6)),
]
LEV5_IDS = set(c.id for c in LEV5_TABLE) | {"full-200x40x128-generic-i8s6", "full-965x193x3-large-i8s6"}

# ---- the ragged pair block as tiles of its own (k_assemble_i8_tail): (300, D, 130), option i8_tail = 1 against 0 --------------------------
# D -> (full 128-pair blocks, 32-pair blocks of the rest, pairs in the last of them)
TAIL_D = {9: (0, 2, 13), 47: (8, 4, 8), 49: (9, 3, 9), 63: (15, 3, 32)}
TAIL_CASES = {t: [_case("tail%d" % t, 300, _D, 130, "%d pairs = %d x 128 + %d x 32 (last holds %d)" % ((_D * (_D + 1) // 2,) + TAIL_D[_D]),
                        flags=I8(6), options={"medium": 0, "i8_tail": t}) for _D in TAIL_D] for t in (0, 1)}


# ---- the plan a case must get ---------------------------------------------------------------------------------------------------------------
def check_plan(case):
    """the planning rule (csrc/plan.h through the probe) sends the case where its table says; returns the plan"""
    p = plan(case.M, case.D, case.n, case.flags, **case.options)
    want = {"fused": (1, 0, 0), "medium": (0, 1, 0), "generic": (0, 0, 0), "large": (0, 0, 1)}[case.path]
    assert (p["fused"], p["medium"], p["big"]) == want, (case.id, p)
    S = slices(case)
    assert bool(p["i8_requested"]) == bool(S) and p["i8S"] == S, (case.id, p)
    assert p["Mp"] == (case.M + 63) // 64 * 64 and p["NB"] == (4 if case.D > 64 else (case.D + 15) // 16), (case.id, p)
    if case.M <= 17:                     # the clamp of nsplit to the 16-row units of Mp is reached
        assert p["nsplit"] == p["Mp"] // 16 == 4, (case.id, p)
    if case.path == "large":
        assert p["nbk"] == (case.D + 63) // 64, (case.id, p)
        if S:
            assert p["gbase"], (case.id, p)
    if S:
        assert p["i8_nks"] == (case.M + 31) // 32 and p["NP"] == case.D * (case.D + 1) // 2 and p["nCp"] == (case.n + 127) // 128 * 128, (case.id, p)
        assert (p["i8_bn"], i8_geometry(case)["WN"]) == ((64, 2) if S == 7 else (128, 4)), (case.id, p)
        # which leverage GEMM the case runs (`edges` prints it): the int8 row-count cases, which caught the trace term 3e-11 cond(G) off
        # the oracle when it was summed from 5 of 6 slices, keep every slice; the cases added for the 5-slice form do run it
        if case.table == "i8m":
            assert p["i8_lev_full"], (case.id, p)
        if case.id in LEV5_IDS:
            assert not p["i8_lev_full"], (case.id, p)
    if "fsplit" in case.options:
        assert p["fsplit"] == case.options["fsplit"] > 1 and p["nsplit"] >= p["fsplit"], (case.id, p)
    elif case.table == "full" and case.path == "generic" and not S:
        assert p["fsplit"] == 1, (case.id, p)
    return p


def i8_geometry(case):
    from plan_probe import probe
    r = probe(case.M, case.D, case.n, case.flags, options=case.options)
    assert r["check"]["code"] == 0 and r["option_error"] is None, r
    return r["i8"]


def edges(case, p=None):
    """one line: the figures a reader needs to see which edge the case sits on, from the plan itself"""
    p = p or check_plan(case)
    s = "NB %d (%d of %d columns)" % (p["NB"], case.D, p["DP"])
    if p["big"]:
        s += ", %d column blocks" % p["nbk"]
    s += ", M %d of Mp %d, nsplit %d, fsplit %d" % (case.M, p["Mp"], p["nsplit"], p["fsplit"])
    s += ", %d chains = %d x 16 + %d" % (case.n, case.n // 16, case.n % 16)
    if case.path == "medium":
        s += ", k_step_medium<%d,%d>" % medium_variant(case.M, case.D)
    if slices(case):
        s += ", S %d, %d k-stages, %d pairs = %d x %d + %d, chains padded to %d" % (p["i8S"], p["i8_nks"], p["NP"], p["NP"] // p["i8_bn"], p["i8_bn"],
                                                                                  p["NP"] % p["i8_bn"], p["nCp"])
        if p["i8S"] == 6:
            s += ", leverages from %d slices" % (6 if p["i8_lev_full"] else 5)
    return s


# ---- inputs and the battery -------------------------------------------------------------------------------------------------------------------
def data_of(case):
    return synthetic_logreg(case.M, case.D, DATA_SEED)


def context(lib, case):
    """a context of `lib` for the case with its data; the oracle gets the flags it knows (it is fp64 throughout and has no options)"""
    if lib.on_gpu:
        ctx = lib.context(case.M, case.D, case.n, flags=case.flags, options=case.options or None)
    else:
        ctx = lib.context(case.M, case.D, case.n, flags=case.flags & (_capi.COMPAT | _capi.FLAG_MMALA_FULL))
    ctx.set_data(*data_of(case), ALPHA)
    return ctx


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


_inputs, _oracle_out = {}, {}


def inputs(case, oracle):
    """The fixed arguments of the battery.  The momentum of `leapfrog` and `metric_terms` is p = chol(G(w)) z with the oracle's own
    metric: a fixed-scale p diverges when M < D, where the metric is dominated by the prior."""
    key = (case.M, case.D, case.n, case.flags & _capi.COMPAT)
    if key not in _inputs:
        M, D, n = case.M, case.D, case.n
        rs = np.random.RandomState(1000 * D + M + n)
        w = 0.2 * rs.randn(n, D) / np.sqrt(D)
        z = rs.randn(n, D)
        with context(oracle, case) as ctx:
            G, _, _ = ctx.metric(w)
        p = np.stack([np.linalg.cholesky(G[c]) @ z[c] for c in range(n)])
        ns = rs.randint(0, 3, n).astype(np.int32); ns[0] = 1
        dr = np.where(rs.rand(n) < 0.5, 1, -1).astype(np.int32)
        u_len, g_dir, u_acc = rs.rand(n), rs.randn(n), rs.rand(n)
        _inputs[key] = _freeze(dict(w=w, z=z, p=p, ns=ns, dr=dr, u_len=u_len, g_dir=g_dir, u_acc=u_acc))
    return _inputs[key]


def battery(ctx, i, case):
    """the same calls on either library: {"call.output": array}"""
    out = {}
    with np.errstate(all="ignore"):
        out["log_posterior.ljl"] = ctx.log_posterior(i["w"])
        out["metric.G"], out["metric.hld"], out["metric.grad"] = ctx.metric(i["w"])
        out["metric_terms.tr"], out["metric_terms.q"] = ctx.metric_terms(i["w"], i["p"])
        out["leapfrog.w"], out["leapfrog.p"], out["leapfrog.hld"], out["leapfrog.status"] = ctx.leapfrog(i["w"], i["p"], case.eps, i["dr"], i["ns"], K)
        for k, v in ctx.transition(i["w"], i["z"], i["u_len"], i["g_dir"], i["u_acc"], L=L, eps=case.eps, K=K).items():
            out["transition." + k] = v
        for k, v in ctx.hmc_transition(i["w"], i["z"], i["u_len"], i["u_acc"], L=HMC_L, eps=HMC_EPS).items():
            out["hmc." + k] = v
        for k, v in ctx.mmala_transition(i["w"], i["z"], i["u_acc"], MMALA_EPS).items():
            out["mmala." + k] = v
    return out


def mmala_full(ctx, i):
    with np.errstate(all="ignore"):
        return ctx.mmala_transition(i["w"], i["z"], i["u_acc"], MMALA_EPS)


def oracle_battery(oracle, case):
    """the battery of a case on the oracle (the full-mMALA cases: their one call), once per process, read-only"""
    if case.id not in _oracle_out:
        i = inputs(case, oracle)
        with context(oracle, case) as ctx:
            r = {"mmala." + k: v for k, v in mmala_full(ctx, i).items()} if case.table == "full" else battery(ctx, i, case)
        _oracle_out[case.id] = _freeze(r)
    return _oracle_out[case.id]


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and (np.array_equal(a, b, equal_nan=True) if a.dtype.kind == "f" else np.array_equal(a, b))


# ---- the trace term restated in np.longdouble -------------------------------------------------------------------------------------------------
# tr_d = tr(G^-1 dG/dw_d) = sum_n v_n (1 - 2 p_n) x_nd h_n,  h_n = x_n' G^-1 x_n = |L^-1 x_n|^2,  G = X' diag(v) X + I / alpha = L L'
# (oracle/rmhmc_numpy.py).  For the int8 cases closest to their bound, the oracle's own error against this restatement:
# id -> (cond(G), oracle, library on an MI355X with the 6-slice leverage GEMM; 5 slices); the bound is 1e-9
TR_LONGDOUBLE_CASES = {
    "i8m-33x70x5-large-i8s6": (4.7e3, 6.9e-14, 7.3e-10, 1.2e-7),
    "i8m-1x40x5-generic-i8s6": (1.0e3, 5.4e-14, 4.2e-10, 5.0e-8),
}


def trace_term_longdouble(case, w):
    LD = np.longdouble
    XX, _ = data_of(case)
    X = XX.astype(LD)
    D = case.D
    out = np.zeros((len(w), D), dtype=LD)
    for c in range(len(w)):
        f = X @ w[c].astype(LD)
        p = 1 / (1 + np.exp(-f))
        v = p * (1 - p)
        G = (X.T * v) @ X + np.eye(D, dtype=LD) / LD(ALPHA)
        Lc = np.zeros((D, D), dtype=LD)
        for j in range(D):
            Lc[j, j] = np.sqrt(G[j, j] - Lc[j, :j] @ Lc[j, :j])
            Lc[j + 1:, j] = (G[j + 1:, j] - Lc[j + 1:, :j] @ Lc[j, :j]) / Lc[j, j]
        Y = np.zeros((D, len(X)), dtype=LD)                      # L Y = X'
        for j in range(D):
            Y[j] = (X[:, j] - Lc[j, :j] @ Y[:j]) / Lc[j, j]
        h = (Y * Y).sum(axis=0)
        out[c] = X.T @ (v * (1 - 2 * p) * h)
    return out


def rel_err_longdouble(a, b):
    """conftest's rel_err without the cast to float64"""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
