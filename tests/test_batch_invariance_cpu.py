"""tests/helpers/batch_invariance.py without a GPU: the plan of every case holds still over its sub-batches (so a bit difference on the
GPU is the kernels', not the planning rule's), the harness itself slices inputs, `theta0` and `chain_offset` correctly (the CPU oracle
steps chains one at a time, so on it the comparison must come out equal - and must not when the slicing is off by one), the default
plans do part where DESIGN section 7 says they do, and a sharded job picks its arithmetic from the job."""
import os
import sys

import numpy as np
import pytest

from riemannhamiltonianmontecarlo_amd import _capi, multi_gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import batch_invariance as B  # noqa: E402
import shape_edges as E  # noqa: E402
from plan_probe import probe  # noqa: E402


# ---- 1. the plan ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", B.CASES, ids=B.IDS)
def test_signature_is_the_same_for_the_whole_batch_and_every_sub_batch(case):
    s = B.check_path(case)
    print("%s (%d chains): %s" % (case.id, case.n, B.sig_text(case)))
    counts = sorted(set([b - a for a, b in B.ranges(case)] + list(B.CHAIN_COUNTS) + [b - a for a, b in B.DELTA_RANGES]))
    for n, sig in zip(counts, B.signatures(case, counts)):
        assert sig == s, "%s: the plan moves between %d and %d chains: %s" % (case.id, case.n, n, B.sig_diff(s, sig))


def test_without_the_options_the_plan_does_move():
    """the create options are what holds it still: with the defaults the generic shape gets another nsplit at 2100 chains than at 130
    (at M = 300 the 20 units of 16 rows cap it below 1632 chains), and the one-launch cases leave their path above 512"""
    c = B.BY_ID["generic"]._replace(options={})
    a, b = B.signatures(c, [130, 2100])
    assert "nsplit" in B.sig_diff(a, b), B.sig_diff(a, b)
    c = B.BY_ID["medium_nb2"]
    a, b = B.signatures(c, [512, 513])
    assert "medium" in B.sig_diff(a, b)


def test_sub_batches_cover_the_edges():
    """every chain but the first changes its slot at least once, the first changes its batch size; the remainders of the 16-chain
    groups, 64-chain grids and 128-chain tiles are hit; the permutation moves every chain"""
    for case in B.CASES:
        n, rg = case.n, B.ranges(case)
        assert all(0 <= a < b <= n for a, b in rg), case.id
        moved = np.zeros(n, bool)
        for a, b in rg:
            if a > 0:
                moved[a:b] = True
        assert moved[1:].all(), (case.id, np.nonzero(~moved)[0])
        if n < 81:
            assert (1, n) in rg and (n - 1, n) in rg and any(b - a == 1 and 0 < a < n - 1 for a, b in rg), case.id
        else:
            assert any(a == 0 and b < n for a, b in rg), case.id
        sizes = set(b - a for a, b in rg)
        if n == 81:
            assert {16, 1, 17, 65} <= sizes                       # a full group, one chain, a group and one, a grid and one
        if n == 130:
            assert {128, 3, 1, 129} <= sizes                      # a full tile, a tile's rest, one chain, a tile and one
        p = B.perm(case)
        assert not (p == np.arange(n)).any()


# ---- 2. / 3. the harness on the oracle -------------------------------------------------------------------------------------------------------
CPU_CASES = ["fused", "medium_nb2", "generic", "hmc_traj", "large", "compat"]      # (the int8 flags mean nothing to the oracle)
_whole = {}


def _oracle_whole(oracle, case):
    if case.id not in _whole:
        i = B.inputs(case, oracle)
        with B.context(oracle, case) as ctx:
            out = {"battery": B.battery(ctx, i, case), "chains": B.run_chains(ctx, case, i["w"])}
            for s in B.samplers_of(case, oracle):
                out[s] = B.run_sampler(ctx, s, case, i["w"])
        for d in out.values():
            E._freeze(d)
        _whole[case.id] = out
    return _whole[case.id]


def _oracle_part(oracle, case, rows, theta_shift=0, offset_shift=0):
    """the sub-batch `rows` on the oracle; the shifts plant the two mistakes the harness could make"""
    i = B.take(B.inputs(case, oracle), rows)
    a = rows[0]
    th = B.inputs(case, oracle)["w"][a + theta_shift:rows[1] + theta_shift]
    with B.context(oracle, B.sub(case, rows[1] - a)) as ctx:
        out = {"battery": B.battery(ctx, i, case), "chains": B.run_chains(ctx, case, th, a + offset_shift)}
        for s in B.samplers_of(case, oracle):
            out[s] = B.run_sampler(ctx, s, case, th, a + offset_shift)
    return out


@pytest.mark.parametrize("cid", CPU_CASES)
def test_harness_on_the_oracle(oracle, cid):
    """battery, samplers and the timed path on every sub-batch equal the rows of the whole batch bit for bit; so does the permuted batch
    for the battery"""
    case = B.BY_ID[cid]
    whole = _oracle_whole(oracle, case)
    for k, v in whole["battery"].items():
        if v.dtype.kind == "f":
            assert np.isfinite(v).all(), (cid, k)
    for rows in B.ranges(case):
        part = _oracle_part(oracle, case, rows)
        for call in whole:
            assert B.bits_differ(whole[call], part[call], rows) == [], (cid, rows, call)
    p = B.perm(case)
    with B.context(oracle, case) as ctx:
        permuted = B.battery(ctx, B.take(B.inputs(case, oracle), p), case)
    assert B.bits_differ(whole["battery"], permuted, p) == [], cid


@pytest.mark.parametrize("cid", ["generic", "hmc_traj"])
def test_harness_notices_a_shifted_theta0_and_a_chain_offset_off_by_one(oracle, cid):
    """the negative control: `theta0` one row off changes every sampler's samples, `chain_offset` one off changes the draws"""
    case = B.BY_ID[cid]
    whole = _oracle_whole(oracle, case)
    rows = (16, 33) if case.n == 81 else B.ranges(case)[1]
    for shift in (dict(theta_shift=1), dict(offset_shift=1)):
        part = _oracle_part(oracle, case, rows, **shift)
        assert B.bits_differ(whole["battery"], part["battery"], rows) == []          # (explicit inputs: neither enters)
        for call in whole:
            if call != "battery":
                bad = B.bits_differ(whole[call], part[call], rows)
                assert any(b.startswith("samples:") or b.startswith("w:") for b in bad), (cid, shift, call, bad)


def test_comparator_sees_one_bit_and_a_nan_payload():
    a = {"x": np.linspace(1, 2, 12).reshape(4, 3), "k": np.arange(4, dtype=np.int32)}
    b = B.take(a, (1, 3))
    assert B.bits_differ(a, b, (1, 3)) == []
    b["x"][1, 2] = np.nextafter(b["x"][1, 2], 3.0)
    bad = B.bits_differ(a, b, (1, 3))
    assert len(bad) == 1 and bad[0].startswith("x: 1 of 2 chains differ, first at row 1"), bad
    c = B.take(a, (1, 3)); c["x"][0, 0] = np.nan
    w = {"x": a["x"].copy(), "k": a["k"]}; w["x"][1, 0] = np.nan
    assert B.bits_differ(w, c, (1, 3)) == []                                         # the same NaN is equal
    c["x"][0, 0] = -np.nan
    assert B.bits_differ(w, c, (1, 3)) != []                                         # another NaN is not
    z = B.take(a, (1, 3)); z["k"][0] += 1
    assert B.bits_differ(a, z, (1, 3))[0].startswith("k: 1 of 2")


# ---- 4. where the default plans part ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", B.THRESHOLDS, ids=[r["id"] for r in B.THRESHOLDS])
def test_default_plans_of_a_job_and_of_its_shards_differ_where_design_says(row):
    job, shard = B.default_plans(row["M"], row["D"], row["n"], row["shard"], auto=row.get("auto", False))
    assert multi_gpu.shard_range(row["n"], 2, 0) == (0, row["shard"])
    for k, want in row["differ"].items():
        assert (job["plan"][k], shard["plan"][k]) == want, (row["id"], k, job["plan"][k], shard["plan"][k])
    for k in row["same"]:
        assert job["plan"][k] == shard["plan"][k], (row["id"], k)


def test_default_plans_at_the_shapes_the_gpu_test_runs():
    for name, (M, D, n, shard, differ) in B.GPU_THRESHOLDS.items():
        job, part = B.default_plans(M, D, n, shard)
        for k, want in differ.items():
            assert (job["plan"][k], part["plan"][k]) == want, (name, k, job["plan"][k], part["plan"][k])
    # the fsplit pair: the row ranges of the assembly (with their planes) and the row splits of the 16-chain passes (30 against 40),
    # nothing else but the chain count; G is summed by the assembly alone
    M, D, n, shard, _ = B.GPU_THRESHOLDS["fsplit"]
    job, part = B.default_plans(M, D, n, shard)
    diff = {k for k in job["plan"] if job["plan"][k] != part["plan"][k]}
    assert diff == {"n", "fsplit", "gpart_planes", "nsplit"}, diff
    assert (job["plan"]["nsplit"], part["plan"]["nsplit"]) == (30, 40)
    M, D, n, shard, _ = B.GPU_THRESHOLDS["medium"]
    job, part = B.default_plans(M, D, n, shard)
    diff = {k for k in job["plan"] if job["plan"][k] != part["plan"][k]}
    assert diff == {"n", "medium", "medium_lds"}, diff            # (Mp = 320: the 20 units of 16 rows cap nsplit on both sides)


def test_amh_block_size_switches_at_1024_chains():
    M, big, small = B.AMH_THRESHOLD
    a, b = probe(M, 5, big)["amh"], probe(M, 5, small)["amh"]
    assert (a["nt"], b["nt"]) == (64, 256) and (a["rows"], b["rows"]) == ((M + 63) // 64, (M + 255) // 256), (a, b)
    assert probe(M, 5, 1023)["amh"] == b and probe(1025, 5, big)["amh"]["nt"] == 256


# ---- a sharded job takes its arithmetic from the job -------------------------------------------------------------------------------------------
def test_shard_flags_are_a_function_of_the_job():
    """700 chains at (1000, 40): the job is large enough for the int8 metric, a shard of 350 or of 88 would not be on its own"""
    N, D, n = 1000, 40, 700
    i8 = _capi.int8_metric_flags(6) | _capi.FLAG_INT8_CERTIFY
    assert _capi.auto_metric_flags(D, n, M=N) == i8 and _capi.auto_metric_flags(D, 350, M=N) == 0
    for sampler, want in (("RMHMC", _capi.COMPAT | i8), ("mMALA", i8), ("IWLS", i8), ("HMC", 0), ("AMH", 0), ("Gibbs", 0)):
        assert multi_gpu.shard_flags(sampler, D, n, N, compat=True) == want, sampler
    assert multi_gpu.shard_flags("RMHMC", D, n, N, compat=False) == i8


class _Stop(Exception):
    pass


class _FakeDist:
    """torch.distributed as sample_sharded sees it before its first context: a world of `world` ranks in which this process is `rank`"""
    class ReduceOp:
        MIN = MAX = SUM = None

    def __init__(self, world, rank):
        self.world, self.rank = world, rank

    def get_rank(self):
        return self.rank

    def get_world_size(self):
        return self.world

    def get_backend(self):
        return "gloo"

    def all_reduce(self, x, op=None):
        pass


class _RecordingLib:
    """stands in for the loaded library: notes what the shard's context is created with, and stops there"""
    on_gpu, has_out, has_diag, has_quant, path = False, True, True, True, "recording"

    def context(self, M, D, n_chains=1, flags=0, device=0, options=None):
        raise _Stop(M, D, n_chains, flags)


@pytest.mark.parametrize("world", [1, 2, 8])
@pytest.mark.parametrize("how", ["RMHMC", "RMHMC-diagnostics", "mMALA", "IWLS", "HMC"])
def test_every_rank_of_a_sharded_job_gets_the_jobs_flags(monkeypatch, world, how):
    """both call sites of sample_sharded: every rank of a 700-chain job at (1000, 40) creates its context with the int8 flags of the
    job, for world sizes 1, 2 and 8, although no shard but the whole job would choose them for itself"""
    N, D, n = 1000, 40, 700
    XX, t = np.zeros((N, D)), np.zeros(N)
    sampler = how.split("-")[0]
    i8 = _capi.int8_metric_flags(6) | _capi.FLAG_INT8_CERTIFY
    want = {"RMHMC": _capi.COMPAT | i8, "mMALA": i8, "IWLS": i8, "HMC": 0}[sampler]
    seen = []
    for rank in range(world):
        monkeypatch.setattr(multi_gpu, "_dist", lambda: _FakeDist(world, rank))
        with pytest.raises(_Stop) as e:
            multi_gpu.sample_sharded(XX, t, n, NumOfIterations=12, BurnIn=4, lib=_RecordingLib(), sampler=sampler,
                                     diagnostics=how.endswith("diagnostics"))
        M_, D_, n_local, flags = e.value.args
        a, b = multi_gpu.shard_range(n, world, rank)
        assert (M_, D_, n_local) == (N, D, b - a)
        seen.append(flags)
    assert seen == [want] * world, (how, world, [hex(f) for f in seen])
