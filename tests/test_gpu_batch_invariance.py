"""A chain's draws do not depend on the batch it runs in: every stepping path once as a whole batch and once in pieces.

The cases, sub-batches, inputs and calls are those of tests/helpers/batch_invariance.py; tests/test_batch_invariance_cpu.py shows
without a GPU that the plan of every case is the same for the whole batch and every sub-batch (create options nsplit_max = 4,
fsplit = 1), so whatever differs here differs in the kernels or in the host code that launches them.  Every comparison of items 1 to 5
is BITWISE (`tobytes`: NaN payloads and the sign of zero count); there is no tolerance in them.

  1. battery: log_posterior, metric, metric_terms, leapfrog, transition, hmc_transition, mmala_transition; every sub-batch [a, b) in a
     context of b - a chains equals rows [a, b) of the whole batch, and the permuted batch equals the permuted outputs.
  2. samplers: sample, hmc_sample, mmala_sample and, through sample_to, amh, iwls, gibbs (D <= 64); 12 iterations, 4 burn-in; sub-batches
     at chain_offset BASE + a with theta0 rows [a, b); samples and every counter; with the default run-time options (graph replay, work
     sorting, cdyn, crestore) and again with graph = 0, sorted = 0.
  3. the timed path: chains_init, chains_run(3), chains_run(4), chains_state on the generic and the 6-slice int8 case.
  4. the delta assemblies pick their slice count S' from the largest difference over the LAUNCH: a batch whose chain 0 moves much
     further than the rest against sub-batches without it - other S', same bits.
  5. the comparator has teeth: the fp64 assembly in two row ranges against one changes the last bits of G, and that is reported.
  6. what sharding really gives where the DEFAULT plans part (one-launch step against generic kernels at 512 chains, one row range
     against two at 1024, k_amh's block size at 1024): equal decisions, continuous outputs to the bounds the existing tests of those
     pairs of paths assert, and both sides against the oracle at the same bounds.

Plan signature per case (batch_invariance.sig_text; all cases Mp 320, nsplit 4, fsplit 1, amh (256, 2)):
  fused          fused  NB 1, hmc_traj        medium_nb1 / nb2  one-launch step NB 1 / 2, hmc_traj      hmc_traj  as medium_nb2
  generic_nb2    generic NB 2                 generic, compat   generic NB 3
  i8s4/5/6       generic NB 3, bn 128, nks 10, NP 820, ksplit 1/3, tail_acc 1, tail_pieces 8      i8s7  bn 64, no tail
  large          large NB 4                   large_i8          large NB 4, i8S 6, NP 2485, ksplit 1/1, tail_acc 1, gbase 1

Seen on an MI355X.  Items 1 to 4: no output of any case differs in a single bit; no assertion had to be narrowed.  Item 4, delta
assemblies of one two-step leapfrog call by S' (end: 4, 5, 6 slices; inner: 4, 5), chain 0's momentum times 6:
  i8s6      whole batch end [0, 1, 1] inner [0, 2];  [1, 130) and [1, 65): end [2, 0, 0] inner [2, 0]
  large_i8  whole batch end [0, 0, 2] inner [0, 2];  [1, 130) and [1, 65): end [2, 0, 0] inner [2, 0]
(scaled chain against the oracle 3e-12 and 9e-12 on theta, the others 9e-14 and 5e-13).  Item 6, whole batch against its two shards:
(300, 20) 514 / 257 chains w_prop 5e-16, H_prop 3e-16, G equal, bits NOT equal; (600, 40) 1100 / 550 (fsplit 1 / 2, nsplit 30 / 40)
w_prop 8e-16, H_prop 3e-16, G 2.5e-15, bits NOT equal; AMH (300, 6) 1024 / 512 chains: equal bits over these five iterations.

Needs an MI355X: run with  pytest -m gpu."""
import os
import sys

import numpy as np
import pytest

from conftest import rel_err
from riemannhamiltonianmontecarlo_amd import _capi
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg
from test_amh_cpu import amh_numpy, philox_draws
from test_gpu_parity import TOL_TRAJ

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import batch_invariance as B  # noqa: E402
import shape_edges as E  # noqa: E402
from sampler_edges import amh_follow  # noqa: E402

pytestmark = pytest.mark.gpu

_case = pytest.mark.parametrize("case", B.CASES, ids=B.IDS)


def _open(hip, case):
    """a context of the case, on the path and with the options the case is for"""
    ctx = B.context(hip, case)
    info = ctx.device_info().split("; options:")[0]
    fused, medium, big, _, S = B.PATHS[case.id]
    for flag, text in ((fused, "fused small-problem path"), (medium, "one-launch step"), (big, "blocked large-D path")):
        assert (text in info) == bool(flag), (case.id, case.n, info)
    if S:
        assert "int8 metric path %d slices: active" % S in info and ctx.int8_certificate()[1], (case.id, info)
    opt = ctx.options()
    assert (opt["nsplit_max"], opt["fsplit"]) == (4, 1), opt
    return ctx


def _check(bad, what):
    assert not bad, "%s: %s" % (what, "; ".join(bad))


# ---- 1. the battery -------------------------------------------------------------------------------------------------------------------
@_case
def test_battery_of_a_sub_batch_equals_the_rows_of_the_whole_batch(hip, oracle, case):
    i = B.inputs(case, oracle)
    with _open(hip, case) as ctx:
        whole = B.battery(ctx, i, case)
        p = B.perm(case)
        permuted = B.battery(ctx, B.take(i, p), case)
    for k, v in whole.items():
        if v.dtype.kind == "f":
            assert np.isfinite(v).all(), (case.id, k)
    bad = ["permuted: " + b for b in B.bits_differ(whole, permuted, p)]
    for rows in B.ranges(case):
        with _open(hip, B.sub(case, rows[1] - rows[0])) as ctx:
            part = B.battery(ctx, B.take(i, rows), case)
        bad += ["[%d, %d): %s" % (rows + (b,)) for b in B.bits_differ(whole, part, rows)]
    _check(bad, case.id)


# ---- 2. the samplers ------------------------------------------------------------------------------------------------------------------
RUN_OPTIONS = {"defaults": {}, "no_graph_unsorted": {"graph": 0, "sorted": 0}}


def _samplers(ctx, case, theta0, a, run_options):
    for k, v in run_options.items():
        ctx.set_option(k, v)
    opt = ctx.options()
    for k in ("graph", "sorted", "cdyn", "crestore"):
        assert opt[k] == run_options.get(k, 1), opt
    return {s: B.run_sampler(ctx, s, case, theta0, a) for s in B.samplers_of(case, ctx.rl)}


@pytest.mark.parametrize("run", list(RUN_OPTIONS))
@_case
def test_samplers_on_a_sub_batch_equal_the_rows_of_the_whole_batch(hip, oracle, case, run):
    th = B.inputs(case, oracle)["w"]
    with _open(hip, case) as ctx:
        whole = _samplers(ctx, case, th, 0, RUN_OPTIONS[run])
    moved = {s: float(np.mean(r["samples"][:, -1] != r["samples"][:, 0])) for s, r in whole.items()}
    print("%s %s: share of coordinates that moved between the first and the last kept iteration: %s" % (case.id, run, moved))
    for s, r in whole.items():
        assert moved[s] > 0.0, (case.id, s)                  # (the chains do move: equal samples are no accident)
        if s != "gibbs":                                     # (a Gibbs chain that stops where the reference would is NaN from there on)
            assert np.isfinite(r["samples"]).all(), (case.id, s)
    bad = []
    for a, b in B.ranges(case):
        with _open(hip, B.sub(case, b - a)) as ctx:
            part = _samplers(ctx, case, th[a:b], a, RUN_OPTIONS[run])
        for s in whole:
            bad += ["%s [%d, %d): %s" % (s, a, b, d) for d in B.bits_differ(whole[s], part[s], (a, b))]
    _check(bad, case.id)


# ---- 3. the timed path ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["generic", "i8s6"])
def test_timed_path_on_a_sub_batch_equals_the_rows_of_the_whole_batch(hip, oracle, cid):
    case = B.BY_ID[cid]
    th = B.inputs(case, oracle)["w"]
    with _open(hip, case) as ctx:
        whole = B.run_chains(ctx, case, th)
    # (chains_run counts leapfrog steps: after 3 + 4 of them, with trajectories of 1 to 3 steps, every chain has finished at least two
    #  transitions, and not all the same number)
    assert np.isfinite(whole["w"]).all() and (whole["iters"] >= 2).all() and len(set(whole["iters"].tolist())) > 1 and whole["accepted"].sum() > 0
    bad = []
    for a, b in B.ranges(case):
        with _open(hip, B.sub(case, b - a)) as ctx:
            part = B.run_chains(ctx, case, th[a:b], a)
        bad += ["[%d, %d): %s" % (a, b, d) for d in B.bits_differ(whole, part, (a, b))]
    _check(bad, cid)


# ---- 4. the slice count of the delta assemblies ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(B.DELTA_SCALE))
def test_delta_assemblies_pick_another_slice_count_and_give_the_same_bits(hip, oracle, cid):
    """S' is picked from max |N_new - N_old| over all chains of the launch (i8_delta_pick, csrc/metric_i8.hip.h): with chain 0's
    momentum scaled the whole batch sums its differences from more slices than a sub-batch without that chain.  The slices a smaller
    difference leaves out are zero, so the integers - and the bits of every common chain - are the same."""
    case = B.BY_ID[cid]
    i = B.delta_batch(case, oracle, B.DELTA_SCALE[cid])
    with B.context(oracle, case) as ctx:
        ref = B.delta_leapfrog(ctx, i, case)
    assert all(np.isfinite(ref[k]).all() for k in ("w", "p", "hld")) and not ref["status"].any(), cid     # finite in the oracle
    with _open(hip, case) as ctx:
        whole = B.delta_leapfrog(ctx, i, case)
        counts = {"whole": ctx.i8_delta_counts()}
    assert np.isfinite(whole["w"]).all() and not whole["status"].any()
    print("%s: against the oracle: theta of the scaled chain %.1e, of the others %.1e" % (cid, rel_err(whole["w"][0], ref["w"][0]),
                                                                                     rel_err(whole["w"][1:], ref["w"][1:])))
    assert rel_err(whole["w"][1:], ref["w"][1:]) < TOL_TRAJ              # (the bound of int8 trajectories at 6 slices)
    bad = []
    for rows in B.DELTA_RANGES:
        with _open(hip, B.sub(case, rows[1] - rows[0])) as ctx:
            part = B.delta_leapfrog(ctx, B.take(i, rows), case)
            counts[rows] = ctx.i8_delta_counts()
        bad += ["[%d, %d): %s" % (rows + (b,)) for b in B.bits_differ(whole, part, rows)]
    print("%s: delta assemblies by S' (end: 4, 5, 6; inner: 4, 5): %s" % (cid, counts))
    for rows in B.DELTA_RANGES:
        for k in ("end", "inner"):                                       # as many delta assemblies in either, and there are some
            assert sum(counts[rows][k]) == sum(counts["whole"][k]) > 0, counts
        assert counts[rows] != counts["whole"], "the scaled chain did not change the slice count: %s" % counts
    _check(bad, cid)


# ---- 5. the comparator has teeth ------------------------------------------------------------------------------------------------------
def test_comparator_reports_the_last_bit_change_of_another_row_split(hip, oracle):
    """the generic case at M = 600 (Mp = 640: two row ranges of the fp64 assembly are possible): fsplit = 2 against fsplit = 1 is the
    known last-bit change of test_small_batch_row_split_of_the_fp64_assembly, and the helper must report it"""
    case = B.BY_ID["generic"]._replace(M=600)
    w = B.inputs(case, oracle)["w"]
    out = {}
    for fs in (1, 2):
        c = case._replace(options=dict(case.options, fsplit=fs))
        with B.context(hip, c) as ctx:
            assert ctx.get_option("fsplit") == fs
            G, hld, grad = ctx.metric(w)
        out[fs] = {"G": G, "hld": hld, "grad": grad}
    bad = B.bits_differ(out[1], out[2], (0, case.n))
    print(bad)
    assert any(b.startswith("G: ") for b in bad), bad
    assert rel_err(out[2]["G"], out[1]["G"]) < 1e-14
    assert B.bits_differ(out[1], B.take(out[1], (5, 9)), (5, 9)) == []


# ---- 6. where the default plans part ----------------------------------------------------------------------------------------------------
def _follow(n, shard):
    """the chains the oracle follows: both ends of the batch and of each shard, and a few spread over it"""
    return np.unique(np.concatenate([[0, 1, shard - 1, shard, shard + 1, n - 1], np.linspace(2, n - 2, 26).astype(int)]))


def _transition_inputs(D, n, seed):
    rs = np.random.RandomState(seed)
    return dict(w=0.2 * rs.randn(n, D) / np.sqrt(D), z=rs.randn(n, D), u_len=rs.rand(n), g_dir=rs.randn(n), u_acc=rs.rand(n))


def _transition(ctx, i):
    with np.errstate(all="ignore"):
        return ctx.transition(i["w"], i["z"], i["u_len"], i["g_dir"], i["u_acc"], L=E.L, eps=0.4, K=E.K)


def _assert_transitions_agree(a, b, what):
    """the assertions of test_medium_one_launch_step_matches_generic_and_oracle"""
    for k in ("nsteps", "accepted"):
        assert np.array_equal(a[k], b[k]), (what, k)
    assert np.array_equal(a["status"] != 0, b["status"] != 0), what
    for k in ("w_prop", "p_prop", "w", "hld_prop"):
        assert rel_err(a[k], b[k]) < TOL_TRAJ, (what, k, rel_err(a[k], b[k]))
    assert rel_err(a["H_prop"], b["H_prop"]) < 1e-8, (what, rel_err(a["H_prop"], b["H_prop"]))


@pytest.mark.parametrize("name", list(B.GPU_THRESHOLDS))
def test_shards_with_another_default_plan_agree_to_rounding(hip, oracle, name):
    """DEFAULT options.  (300, 20): 514 chains run the generic kernels, shards of 257 the one-launch step; (600, 40): 1100 chains
    assemble G over one row range, shards of 550 over two.  One transition from explicit inputs: decisions and status equal, continuous
    outputs to TOL_TRAJ (1e-8 on H), G to 1e-14 for the row ranges; each side against the oracle at the same bounds on the followed
    chains."""
    M, D, n, shard, _ = B.GPU_THRESHOLDS[name]
    XX, t = synthetic_logreg(M, D, E.DATA_SEED)
    i = _transition_inputs(D, n, 9)

    def run(lib, rows):
        ii = B.take(i, rows)
        with lib.context(M, D, len(ii["w"]), flags=0) as ctx:
            ctx.set_data(XX, t, E.ALPHA)
            if lib.on_gpu:
                info = ctx.device_info().split("; options:")[0]
                if name == "medium":
                    assert ("one-launch step" in info) == (len(ii["w"]) <= 512), info
            r = _transition(ctx, ii)
            r["G"] = ctx.metric(ii["w"])[0]
        return r

    whole = run(hip, (0, n))
    parts = [run(hip, (0, shard)), run(hip, (shard, n))]
    sharded = {k: np.concatenate([p[k] for p in parts]) for k in whole}
    ids = _follow(n, shard)
    ref = run(oracle, ids)
    print("%s: %d chains, %d accepted, nsteps %s; whole against shards: w_prop %.1e, H_prop %.1e, G %.1e; bits equal: %s" % (
        name, n, whole["accepted"].sum(), np.bincount(whole["nsteps"]).tolist(), rel_err(sharded["w_prop"], whole["w_prop"]),
        rel_err(sharded["H_prop"], whole["H_prop"]), rel_err(sharded["G"], whole["G"]), not B.bits_differ(whole, sharded, (0, n))))
    assert 0 < whole["accepted"].sum() and len(set(whole["nsteps"].tolist())) > 1
    _assert_transitions_agree(sharded, whole, name + ": shards against the whole batch")
    assert rel_err(sharded["G"], whole["G"]) < 1e-14
    for side, r in (("whole batch", whole), ("shards", sharded)):
        _assert_transitions_agree(B.take(r, ids), ref, "%s: %s against the oracle" % (name, side))
        assert rel_err(r["G"][ids], ref["G"]) < 1e-12, side       # (G against the oracle: the bound of tests/test_gpu_shape_edges.py)


def test_amh_shards_below_1024_chains_agree_to_rounding(hip):
    """amh_shape: 1024 chains run one wavefront per chain, two shards of 512 a 256-thread workgroup per chain - other row sums.  Five
    iterations: accept counts and the final ProposalSD equal, samples to the 1e-10 tests/test_gpu_amh.py asserts against the NumPy
    restatement; both sides against the restatement on the followed chains."""
    M, n, shard = B.AMH_THRESHOLD
    D, T, Bn, seed = 6, 5, 2, 23
    XX, t = synthetic_logreg(M, D, E.DATA_SEED)

    def run(n_ctx, offset):
        with hip.context(M, D, n_ctx, flags=0) as ctx:
            ctx.set_data(XX, t)
            smp, acc, sd, _ = ctx.amh_sample(T, Bn, seed=seed, chain_offset=offset)
        return {"samples": smp, "accepted": acc, "sd": sd}

    whole = run(n, 0)
    parts = [run(shard, 0), run(shard, shard)]
    sharded = {k: np.concatenate([p[k] for p in parts]) for k in whole}
    ids = amh_follow(n)
    ids = np.unique(np.concatenate([ids, [shard - 1, shard]]))
    ref = amh_numpy(XX, t, T, Bn, philox_draws(seed, ids, D), n=len(ids))
    print("amh: whole against shards %.1e; bits equal: %s" % (rel_err(sharded["samples"], whole["samples"]), not B.bits_differ(whole, sharded, (0, n))))
    assert np.array_equal(sharded["accepted"], whole["accepted"]) and np.array_equal(sharded["sd"], whole["sd"])
    assert rel_err(sharded["samples"], whole["samples"]) <= 1e-10
    for side, r in (("whole batch", whole), ("shards", sharded)):
        assert np.isfinite(r["samples"]).all(), side
        assert np.array_equal(r["accepted"][ids], ref["accepted"].sum(axis=(1, 2))), side
        assert rel_err(r["samples"][ids], ref["w"][:, Bn:]) <= 1e-10, side
        assert np.array_equal(r["sd"][ids], ref["sd"]), side
