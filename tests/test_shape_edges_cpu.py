"""The cases of tests/helpers/shape_edges.py without a GPU: every case is planned onto the stepping path and kernel variant it exists
for (csrc/plan.h through the probe), and the CPU oracle alone runs the whole battery on it with every output finite, every status 0
(the RMHMC_COMPAT cases apart) and every chain taking at least one step.  That is the condition under which
tests/test_gpu_shape_edges.py leaves nothing out: it has no skip and filters no chain."""
import os
import sys

import numpy as np
import pytest

from riemannhamiltonianmontecarlo_amd import _capi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import shape_edges as E  # noqa: E402

ALL = E.CASES + E.MMALA_FULL_CASES
IDS = [c.id for c in ALL]


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_case_is_planned_onto_its_path(case):
    p = E.check_plan(case)
    print("%s: %s; %s" % (case.id, case.why, E.edges(case, p)))
    if case.path == "medium":
        NB, R = E.medium_variant(case.M, case.D)
        assert NB == p["NB"] and 8 * (64 * 66 + 32 * 34 + 4 * (16 * NB) ** 2 + 2 * p["Mp"] + 12 * 32 + 4 * 40) == p["medium_lds"], (case.id, p)
        if (case.M, case.D, case.n) in E.MEDIUM_VARIANTS:
            assert (NB, R) == E.MEDIUM_VARIANTS[(case.M, case.D, case.n)], case.id
    if case.table == "m" and case.path == "medium":
        assert E.medium_variant(case.M, case.D) == (1, 1)


def test_tables_hold_the_edges_they_are_for():
    """the shapes of the tables, and that the one-launch cases reach the four instantiations no earlier shape does"""
    by = lambda t: sorted(set((c.M, c.D, c.n) for c in E.TABLES[t]))
    assert by("d") == [(300, D, 18) for D in (9, 16, 17, 31, 32, 47, 49, 63)]
    assert by("large") == [(300, D, 3) for D in (127, 128, 129, 191, 193, 255)]
    assert by("m") == sorted((M, D, 5) for M in (1, 15, 16, 17, 63, 65) for D in (5, 12, 40, 70))
    assert by("i8m") == sorted((M, D, 5) for M in (1, 31, 32, 33) for D in (40, 70))
    assert sorted((c.n, E.slices(c)) for c in E.TABLES["n"]) == sorted([(n, 0) for n in (1, 16, 17, 64, 65)] + [(n, 6) for n in (1, 16, 17, 127, 128)])
    reached = set(E.medium_variant(c.M, c.D) for c in E.CASES if c.path == "medium")
    assert {(1, 4), (1, 0), (2, 1), (2, 2)} <= reached, reached
    assert set(c.path for c in E.CASES) == {"fused", "medium", "generic", "large"}
    assert sorted(set(E.slices(c) for c in E.TABLES["d"])) == [0, 4, 5, 6, 7]
    # D = 255 (and 256): the only shapes without a ragged 128-pair block
    assert [c.D for c in E.TABLES["large"] if E.slices(c) and c.D * (c.D + 1) // 2 % 128 == 0] == [255]


@pytest.mark.parametrize("t", [0, 1])
def test_tail_cases_are_planned_with_and_without_the_tail_kernel(t):
    """option i8_tail = 1 runs the ragged rest as tiles of its own at every D of the table - at D = 9 too, where there is no full block
    and the main launch has no workgroups - and i8_tail = 0 never does"""
    for case in E.TAIL_CASES[t]:
        p = E.check_plan(case)
        g = E.i8_geometry(case)
        full, blocks, last = E.TAIL_D[case.D]
        assert p["ksplit_a"] == 1 and g["nCB"] == 2, (case.id, p, g)
        assert (g["nPBfull"], p["NP"] - 128 * full - 32 * (blocks - 1)) == (full, last), (case.id, p, g)
        if t:
            assert p["tail_acc"] and p["tail_always"] and g["tail"] and (g["ntail"], p["tail_blocks"]) == (blocks, blocks), (case.id, p, g)
            assert g["npb"] == full and g["nblk_main"] == 2 * full and g["pb32_0"] == 4 * full, (case.id, g)
        else:
            assert not p["tail_acc"] and not g["tail"] and g["npb"] == full + 1, (case.id, p, g)


_seen = {"nsteps": set(), "full_rejected": 0, "cases": set()}


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_oracle_runs_the_whole_battery(oracle, case):
    o = E.oracle_battery(oracle, case)
    i = E.inputs(case, oracle)
    assert np.isfinite(i["p"]).all()
    for k, v in o.items():
        if v.dtype.kind == "f":
            assert np.isfinite(v).all(), (case.id, k)
    _seen["cases"].add(case.id)
    if case.table == "full":
        _seen["full_rejected"] += int((o["mmala.accepted"] == 0).sum())
        return
    st = np.concatenate([o["leapfrog.status"], o["transition.status"]])
    if case.flags & _capi.COMPAT:
        assert not (st & (_capi.ST_NOT_PD | _capi.ST_NONFINITE)).any(), (case.id, st)
    else:
        assert not st.any(), (case.id, st)
    assert (o["transition.nsteps"] >= 1).all() and (o["hmc.nsteps"] >= 1).all(), case.id
    assert case.eps == E.EPS, case.id                       # (no int8 row-count case needed a smaller step)
    _seen["nsteps"].update(o["transition.nsteps"].tolist())


def test_over_the_table_the_decisions_vary(oracle):
    """trajectory lengths take more than one value and a full-mMALA proposal is rejected somewhere: equal `nsteps` and `accepted` on
    the GPU are then no accident"""
    for case in ALL:                                          # (cached when the parametrized test ran first)
        if case.id not in _seen["cases"]:
            test_oracle_runs_the_whole_battery(oracle, case)
    assert len(_seen["nsteps"]) >= 2, _seen["nsteps"]
    assert _seen["full_rejected"] >= 1
    acc = np.concatenate([E.oracle_battery(oracle, c)["transition.accepted"] for c in E.CASES])
    print("transition: %d of %d accepted; nsteps %s; full mMALA rejected %d" % (acc.sum(), len(acc), sorted(_seen["nsteps"]), _seen["full_rejected"]))


@pytest.mark.parametrize("cid", list(E.TR_LONGDOUBLE_CASES))
def test_oracle_trace_term_against_longdouble(oracle, cid):
    """The int8 trace terms closest to their 1e-9 bound sit on the worst-conditioned metrics of the tables (M < D).  The oracle's own
    error there, against the np.longdouble restatement, is orders below the bound: cond(G) 2^-53 times a modest factor, held here to
    1e-11.  What the library is off the oracle by is therefore the library's (the grid of the 6-slice leverage GEMM), not the
    reference's."""
    assert np.finfo(np.longdouble).eps < 2e-19
    case = [c for c in E.CASES if c.id == cid][0]
    w = E.inputs(case, oracle)["w"]
    ref = E.trace_term_longdouble(case, w)
    o = E.oracle_battery(oracle, case)["metric_terms.tr"]
    cond = max(np.linalg.cond(G) for G in E.oracle_battery(oracle, case)["metric.G"])
    err = max(E.rel_err_longdouble(o[c], ref[c]) for c in range(case.n))
    print("%s: cond(G) %.1e, oracle trace term against longdouble %.1e" % (cid, cond, err))
    assert err < 1e-11, (cid, err)
