"""The RMHMC core at its tile, block and padding edges, on every stepping path, against the CPU oracle.

The cases are those of tests/helpers/shape_edges.py (each says which kernel variant or remainder it is there for); on every one the
same battery runs on the library and on the oracle: log_posterior, metric, metric_terms, leapfrog (0, 1 and 2 steps, both directions),
transition, hmc_transition, mmala_transition.  tests/test_shape_edges_cpu.py shows without a GPU that every case is planned onto its
path and that the oracle is finite on all of it, so nothing is skipped or filtered here.  Before the battery each case confirms the
stepping path from device_info() and, for the int8 metric, the certificate.

Tolerances are those of the existing tests (test_gpu_parity.py, test_gpu_int8_metric.py, test_mmala.py), per chain with conftest's
rel_err: log posterior and G 1e-12 (G exactly symmetric), half log-det and gradient 1e-11, trace and quadratic term 1e-9 (1e-8 on the
large-D path), leapfrog TOL_STEP where ns <= 1 and TOL_TRAJ otherwise, transition 1e-8 (H_cur 1e-9), HMC 1e-9, mMALA 1e-8 and
1e-6 max(1, |ratio|); the int8 metric G_TOL[S], STEP_TOL[S], 1e3 G_TOL[S] on the trace and quadratic term and on the half log-det,
TOL_TRAJ on trajectories (1e-6 at 4 slices); mMALA w_prop 1e-8 at every slice count.  Where the issue's table names no bound, this
file takes the existing tests' (marked "chosen" in `tolerances`): the int8 half log-det in the absolute form of
test_gpu_int8_metric.py, |hld - oracle| < 1e3 G_TOL[S]; int8 leapfrog chains with two steps at the bound of int8 trajectories, as the
fp64 ones are at TOL_TRAJ; H_cur of the int8 transitions 1e-9 at 6 and 7 slices like test_full_size_config3, the trajectory bound below.

Also here: full mMALA (RMHMC_FLAG_MMALA_FULL, the trace term alone) on every leverage branch, and the ragged pair block as tiles of
its own (k_assemble_i8_tail) at D = 9, 47, 49 and 63, bit-identical to the one-launch form.

Worst error per path and quantity over all cases, measured on an MI355X (the module prints the table after its last test):

  path              ljl    G      hld    grad   tr     q      leapfrog trans. H_prop H_cur  HMC    mMALA w ratio
  fused             5e-16  3e-16  4e-16  5e-16  1e-14  3e-14  3e-15    4e-15  1e-15  7e-16  4e-16  4e-15   4e-14
  medium            1e-15  3e-15  1e-15  2e-15  4e-14  2e-13  7e-15    2e-14  2e-15  1e-15  1e-15  8e-15   2e-12
  generic           1e-15  5e-16  7e-15  2e-15  9e-14  9e-13  1e-13    1e-13  1e-14  5e-15  1e-15  2e-13   3e-12
  large             7e-16  4e-16  7e-15  2e-15  7e-13  5e-13  4e-13    2e-13  2e-14  1e-14  7e-16  2e-13   2e-12
  generic int8 S=4  7e-16  1e-09  6e-09  2e-15  1e-08  3e-09  2e-09    3e-09  6e-11  1e-11  9e-16  3e-09   4e-08
  generic int8 S=5  7e-16  8e-12  2e-11  2e-15  6e-11  1e-11  1e-11    1e-11  3e-13  4e-14  9e-16  2e-11   2e-10
  generic int8 S=6  1e-15  5e-14  3e-11  2e-15  4e-10  7e-12  3e-11    3e-11  1e-12  1e-13  1e-15  2e-11   1e-10
  generic int8 S=7  7e-16  2e-15  6e-14  2e-15  2e-15  2e-15  7e-16    1e-15  5e-16  6e-16  9e-16  2e-15   4e-13
  large int8 S=6    7e-16  5e-14  2e-11  2e-15  7e-10  4e-12  5e-11    4e-11  3e-12  1e-13  7e-16  5e-11   5e-10
(leapfrog: w, p, hld; trans.: w_prop, p_prop, hld_prop, w of `transition`; HMC: every float output.)  Closest to a bound: the int8 trace
term at M < D, 7.3e-10 of 1e-9 at (33, 70, 5) and 4.2e-10 at (1, 40, 5), cond(G) 4700 and 1000; everything else is 6x or more inside.

What the cases found: with the leverages x_n' G^-1 x_n summed from 5 of the 6 slices (the default for S = 6) the trace term of all eight
int8 row-count cases was 2e-8 .. 1.6e-7 off the oracle (bound 1e-9), 1.4e-9 at (300, 255, 3), and the momentum after one step up to
3e-9 (bound 1e-9): 3e-11 cond(G), because G^-1 is cut relative to its largest entry, which is the prior's alpha when M < D.  Shapes with
M < 4 D now keep all slices in the leverage GEMM (csrc/plan.h, Plan::i8_lev_full); the figures above are with that rule.

Needs an MI355X: run with  pytest -m gpu."""
import os
import sys

import numpy as np
import pytest

from conftest import rel_err
from riemannhamiltonianmontecarlo_amd import _capi
from test_gpu_int8_metric import G_TOL, STEP_TOL
from test_gpu_parity import TOL_STEP, TOL_TRAJ

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import shape_edges as E  # noqa: E402

pytestmark = pytest.mark.gpu

_worst = {}    # (path label, quantity) -> (error / tolerance, error, tolerance, case id)


@pytest.fixture(scope="module", autouse=True)
def worst_errors_table():
    """after the module's last test: the error closest to its bound per path and quantity, the table of the module docstring"""
    yield
    for p in sorted(set(p for p, _ in _worst)):
        print("\n" + p)
        for (pp, q), (ratio, e, tol, cid) in sorted(_worst.items()):
            if pp == p:
                print("    %-22s %.1e  (bound %.0e, %s)" % (q, e, tol, cid))


def tolerances(case):
    S, big = E.slices(case), case.path == "large"
    t = {"ljl": 1e-12, "G": 1e-12, "hld": 1e-11, "grad": 1e-11, "tr": 1e-8 if big else 1e-9, "q": 1e-8 if big else 1e-9,
         "step": TOL_STEP, "traj": TOL_TRAJ, "t.prop": 1e-8, "t.H_prop": 1e-8, "t.H_cur": 1e-9,
         "hmc": 1e-9, "mmala.w_prop": 1e-8, "mmala.ratio": 1e-6}
    if S:
        traj = TOL_TRAJ if S >= 5 else 1e-6
        t.update({"G": G_TOL[S], "hld": 1e3 * G_TOL[S], "tr": 1e3 * G_TOL[S], "q": 1e3 * G_TOL[S], "step": STEP_TOL[S], "traj": traj,
                  "t.prop": traj, "t.H_prop": traj,
                  "t.H_cur": 1e-9 if S >= 6 else traj})             # chosen: test_full_size_config3 holds 6 slices to the fp64 bound
    # (hld, "traj" for leapfrog chains with two steps: chosen as well, see the module docstring)
    return t


def label(case):
    S = E.slices(case)
    return case.path + (" int8 S=%d" % S if S else "")


class Report:
    def __init__(self, case):
        self.case, self.bad, self.worst = case, [], {}

    def err(self, name, e, tol, c=None):
        if not e < tol:
            self.bad.append("%s%s %.2e >= %.0e" % (name, "" if c is None else " chain %d" % c, e, tol))
        if e / tol >= self.worst.get(name, (0.0, 1.0, -1.0))[2]:
            self.worst[name] = (e, tol, e / tol)

    def chains(self, name, a, b, tol, rows=None):
        """per chain, conftest's rel_err"""
        for c in (range(len(b)) if rows is None else rows):
            self.err(name, rel_err(a[c], b[c]), tol[c] if isinstance(tol, np.ndarray) else tol, c)

    def same(self, name, a, b):
        if not np.array_equal(a, b):
            self.bad.append("%s differs: %s, oracle %s" % (name, np.asarray(a).tolist(), np.asarray(b).tolist()))

    def finish(self, ctx_info=""):
        case = self.case
        print("%s [%s] %s: %s" % (case.id, label(case), case.why, ", ".join("%s %.1e" % (k, v[0]) for k, v in self.worst.items())))
        for k, (e, tol, ratio) in self.worst.items():
            key = (label(case), k)
            if ratio >= _worst.get(key, (-1.0,))[0]:
                _worst[key] = (ratio, e, tol, case.id)
        assert not self.bad, "%s (%s): %s" % (case.id, case.why, "; ".join(self.bad))


PATH_TEXT = {"fused": "fused small-problem path", "medium": "one-launch step", "large": "blocked large-D path"}   # generic: none of them


def _assert_path(ctx, case):
    """device_info() names the stepping path the case is for and, for the int8 metric, says that it is active; the certificate agrees"""
    info = ctx.device_info().split("; options:")[0]
    for path, text in PATH_TEXT.items():
        assert (text in info) == (path == case.path), (case.id, info)
    S = E.slices(case)
    if S:
        assert "int8 metric path %d slices: active" % S in info, (case.id, info)
        assert ctx.int8_certificate()[1], case.id
    else:
        assert "int8" not in info, (case.id, info)


def _status(r, name, g, o, compat):
    """the documented bits (include/rmhmc.h): under RMHMC_COMPAT the guards may fire and the bits are the oracle's, otherwise the
    pattern of chains that carry any"""
    if compat:
        r.same(name, g & 15, o & 15)
    else:
        r.same(name + " != 0", g != 0, o != 0)


def run_battery_case(hip, oracle, case):
    i = E.inputs(case, oracle)
    o = E.oracle_battery(oracle, case)
    with E.context(hip, case) as ctx:
        _assert_path(ctx, case)
        g = E.battery(ctx, i, case)
    t = tolerances(case)
    S, compat = E.slices(case), bool(case.flags & _capi.COMPAT)
    r = Report(case)
    for k, v in g.items():
        if v.dtype.kind == "f" and not np.isfinite(v).all():
            r.bad.append("%s is not finite" % k)
    if r.bad:
        r.finish()
    r.chains("ljl", g["log_posterior.ljl"], o["log_posterior.ljl"], t["ljl"])
    r.chains("G", g["metric.G"], o["metric.G"], t["G"])
    if not np.array_equal(g["metric.G"], np.swapaxes(g["metric.G"], 1, 2)):
        r.bad.append("G is not exactly symmetric")
    if S:   # (the int8 tests' form: absolute)
        r.err("hld", float(np.abs(g["metric.hld"] - o["metric.hld"]).max()), t["hld"])
    else:
        r.chains("hld", g["metric.hld"], o["metric.hld"], t["hld"])
    r.chains("grad", g["metric.grad"], o["metric.grad"], t["grad"])
    r.chains("tr", g["metric_terms.tr"], o["metric_terms.tr"], t["tr"])
    r.chains("q", g["metric_terms.q"], o["metric_terms.q"], t["q"])
    if case.id in E.TR_LONGDOUBLE_CASES:   # (closest to the bound: where the library stands against the np.longdouble restatement)
        ref = E.trace_term_longdouble(case, i["w"])
        print("%s: trace term against longdouble: library %.1e, oracle %.1e" % (case.id,
              max(E.rel_err_longdouble(g["metric_terms.tr"][c], ref[c]) for c in range(case.n)),
              max(E.rel_err_longdouble(o["metric_terms.tr"][c], ref[c]) for c in range(case.n))))
    # leapfrog: 0, 1 or 2 steps per chain
    ns = i["ns"]
    tol = np.where(ns <= 1, t["step"], t["traj"])
    for k in ("w", "p", "hld"):
        r.chains("leapfrog." + k, g["leapfrog." + k], o["leapfrog." + k], tol)
    still = ns == 0
    if not (E.same_bits(g["leapfrog.w"][still], i["w"][still]) and E.same_bits(g["leapfrog.p"][still], i["p"][still])):
        r.bad.append("leapfrog: a chain with ns = 0 was touched")
    _status(r, "leapfrog.status", g["leapfrog.status"], o["leapfrog.status"], compat)
    # transition
    for k in ("nsteps", "accepted"):
        r.same("transition." + k, g["transition." + k], o["transition." + k])
    _status(r, "transition.status", g["transition.status"], o["transition.status"], compat)
    for k in ("w_prop", "p_prop", "hld_prop", "w"):
        r.chains("transition." + k, g["transition." + k], o["transition." + k], t["t.prop"])
    r.chains("transition.H_prop", g["transition.H_prop"], o["transition.H_prop"], t["t.H_prop"])
    r.chains("transition.H_cur", g["transition.H_cur"], o["transition.H_cur"], t["t.H_cur"])
    # plain HMC
    for k in ("nsteps", "accepted"):
        r.same("hmc." + k, g["hmc." + k], o["hmc." + k])
    for k in ("w_prop", "p_prop", "H_prop", "H_cur", "w"):
        r.chains("hmc." + k, g["hmc." + k], o["hmc." + k], t["hmc"])
    _mmala(r, g, o, t)
    r.finish()


def _mmala(r, g, o, t):
    r.same("mmala.accepted", g["mmala.accepted"], o["mmala.accepted"])
    r.chains("mmala.w_prop", g["mmala.w_prop"], o["mmala.w_prop"], t["mmala.w_prop"])
    for c in range(len(o["mmala.ratio"])):   # (scaled like test_gpu_transition_matches_oracle_synthetic)
        r.err("mmala.ratio", abs(g["mmala.ratio"][c] - o["mmala.ratio"][c]) / max(1.0, abs(o["mmala.ratio"][c])), t["mmala.ratio"], c)


def _table(name):
    return pytest.mark.parametrize("case", E.TABLES[name], ids=[c.id for c in E.TABLES[name]])


@_table("d")
def test_column_tile_edges(hip, oracle, case):
    """(300, D, 18), D = 9 .. 63: NB = 1 .. 4 with exact and ragged last tiles on the generic fp64 kernels, the one-launch step and the
    int8 metric at 6 slices; 4, 5 and 7 slices (the other tile shape) at D = 49 and 63"""
    run_battery_case(hip, oracle, case)


@_table("large")
def test_large_d_block_edges(hip, oracle, case):
    """(300, D, 3), D = 127 .. 255: one short of, exactly and one over two and three 64-column blocks, fp64 and int8; D = 255 has no
    ragged pair block"""
    run_battery_case(hip, oracle, case)


@_table("m")
def test_row_count_edges(hip, oracle, case):
    """M = 1, 15, 16, 17 (below, at and over the 16-row unit nsplit is clamped to), 63 and 65 (around Mp) on the fused kernel, the
    one-launch step, the generic and the large-D kernels"""
    run_battery_case(hip, oracle, case)


@_table("i8m")
def test_int8_row_count_edges(hip, oracle, case):
    """M = 1, 31, 32, 33: one k-stage of 32 rows partly and exactly full, and one row over"""
    run_battery_case(hip, oracle, case)


@_table("n")
def test_chain_count_edges(hip, oracle, case):
    """the whole batch n = 1, 16, 17, 64, 65 (fp64) and 1, 16, 17, 127, 128 (int8)"""
    run_battery_case(hip, oracle, case)


@_table("variant")
def test_one_launch_step_variants(hip, oracle, case):
    """k_step_medium<1,4>, <1,0> and <2,1> (<2,2> is (300, 31, 18) of the D table): the instantiations no other shape of the suite reaches"""
    assert "k_step_medium<%d,%d>" % E.medium_variant(case.M, case.D) == case.why
    run_battery_case(hip, oracle, case)


@_table("lev5")
def test_five_slice_leverages_at_the_large_d_edges(hip, oracle, case):
    """M = 5 D: the leverage GEMM from 5 of 6 slices (what shapes with M >= 4 D run), which the issue's large-D shapes (M = 300 < 4 D)
    do not reach, at three column blocks with one column in the last and at D = 255"""
    run_battery_case(hip, oracle, case)


@_table("compat")
def test_guards_at_the_edges(hip, oracle, case):
    """RMHMC_COMPAT on a ragged NB = 4 shape and on four column blocks: the status bits are the oracle's, guards included"""
    run_battery_case(hip, oracle, case)


@pytest.mark.parametrize("case", E.MMALA_FULL_CASES, ids=[c.id for c in E.MMALA_FULL_CASES])
def test_full_mmala_on_every_leverage_branch(hip, oracle, case):
    """mode 2 of eval_point_phases: k_leverage (one and several row ranges), the int8 leverage GEMM with k_trvec, k_leverage_pair /
    k_trace_big, and the large-D int8 branch; both int8 branches with the 6-slice (M < 4 D) and the 5-slice leverage GEMM"""
    i = E.inputs(case, oracle)
    o = E.oracle_battery(oracle, case)
    with E.context(hip, case) as ctx:
        _assert_path(ctx, case)
        g = {"mmala." + k: v for k, v in E.mmala_full(ctx, i).items()}
    r = Report(case)
    if not (np.isfinite(g["mmala.w_prop"]).all() and np.isfinite(g["mmala.ratio"]).all()):
        r.bad.append("not finite")
        r.finish()
    _mmala(r, g, o, tolerances(case))
    r.chains("mmala.w", g["mmala.w"], o["mmala.w"], tolerances(case)["mmala.w_prop"])
    r.finish()


@pytest.mark.parametrize("D", list(E.TAIL_D))
def test_ragged_pair_block_as_tiles_of_its_own_at_the_block_edges(hip, oracle, D):
    """option i8_tail = 1 against 0 at (300, D, 130): D = 63, the rest exactly three 32-pair blocks; 47 and 49, four and three blocks
    with a padded last one; 9, no full block at all (the main launch has no workgroups).  metric and one leapfrog step are
    bit-identical, and the run with the tail kernel agrees with the oracle."""
    out = {}
    for t in (0, 1):
        case = [c for c in E.TAIL_CASES[t] if c.D == D][0]
        i = E.inputs(case, oracle)
        with E.context(hip, case) as ctx:
            _assert_path(ctx, case)
            assert ctx.get_option("i8_tail") == t
            out[t] = ctx.metric(i["w"]) + ctx.leapfrog(i["w"], i["p"], E.EPS, i["dr"], 1, E.K)
    for k, (a, b) in enumerate(zip(out[0], out[1])):
        assert E.same_bits(a, b), (D, k)
    with E.context(oracle, case) as ctx:
        ref = ctx.metric(i["w"]) + ctx.leapfrog(i["w"], i["p"], E.EPS, i["dr"], 1, E.K)
    r = Report(case)
    G, hld, grad, w1, p1, h1, st = out[1]
    r.chains("G", G, ref[0], G_TOL[6])
    r.err("hld", float(np.abs(hld - ref[1]).max()), 1e3 * G_TOL[6])
    r.chains("grad", grad, ref[2], 1e-11)
    for k, a, b in (("w", w1, ref[3]), ("p", p1, ref[4]), ("hld", h1, ref[5])):
        r.chains("leapfrog." + k, a, b, STEP_TOL[6])
    r.same("leapfrog.status", st, ref[6])
    r.finish()
