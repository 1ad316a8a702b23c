"""csrc/plan.h on the CPU: the argument checks of rmhmc_create, the plan of a context (padding, row splits, the int8 layout, the
stepping path), the launch geometry of the int8 assembly and the AMH variant, asked of the compiled rule through
tests/helpers/plan_probe.cpp.  The expected values were transcribed by hand from the rules as they stood inside rmhmc_create_opts
before plan.h existed; they are not output of the code under test."""
import os
import sys

import pytest

from riemannhamiltonianmontecarlo_amd import _capi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import plan_probe as P  # noqa: E402

I8 = _capi.int8_metric_flags

# name: (M, D, n), then NB DP Mp | nsplit fsplit gpart_planes | medium_lds fused_lds hmc_traj | amh (NT, R)
FULL = {
    "fused": ((150, 6, 5), 1, 16, 192, 12, 1, 0, 0, 23296, 1, 256, 1),
    "medium": ((270, 14, 5), 1, 16, 320, 20, 1, 0, 60160, 0, 1, 256, 2),
    "generic": ((300, 40, 20), 3, 48, 320, 20, 1, 0, 0, 0, 0, 256, 2),
    "generic_rowsplit": ((600, 40, 70), 3, 48, 640, 40, 2, 2, 0, 0, 0, 256, 3),
    "large": ((200, 70, 3), 4, 128, 256, 16, 1, 0, 0, 0, 0, 256, 1),
    "c1": ((690, 15, 1), 1, 16, 704, 44, 2, 2, 66304, 0, 1, 256, 3),
    "c2": ((1000, 8, 1024), 1, 16, 1024, 32, 1, 0, 0, 109824, 1, 64, 16),
    "c3": ((10000, 64, 8192), 4, 64, 10048, 4, 1, 0, 0, 0, 0, 256, 40),
    "c5": ((50000, 256, 4096), 4, 256, 50048, 24, 1, 0, 0, 0, 0, 256, 0),
}
FULL_KEYS = ("NB", "DP", "Mp", "nsplit", "fsplit", "gpart_planes", "medium_lds", "fused_lds", "hmc_traj")

# (M, D, n, flags): the fields the table names
PARTIAL = [
    ((200, 70, 3, 0), dict(nbk=2, npairs=3, big=1)),
    ((50000, 256, 4096, 0), dict(nbk=4, npairs=10, big=1)),
    ((600, 40, 1023, 0), dict(NB=3, DP=48, Mp=640, nsplit=32, fsplit=2, gpart_planes=2)),
    ((600, 40, 1024, 0), dict(nsplit=32, fsplit=1, gpart_planes=0)),
    ((270, 9, 5, 0), dict(medium=1, medium_lds=60160)),
    ((270, 32, 5, 0), dict(NB=2, medium=1, medium_lds=84736)),
    ((270, 33, 5, 0), dict(NB=3, medium=0, medium_lds=0, hmc_traj=0)),
    ((2048, 14, 5, 0), dict(nsplit=64, fsplit=8, gpart_planes=8, medium=1, medium_lds=87808)),
    ((2049, 14, 5, 0), dict(Mp=2112, medium=0, medium_lds=0, hmc_traj=1)),
    ((270, 14, 512, 0), dict(medium=1, medium_lds=60160)),
    ((270, 14, 513, 0), dict(medium=0, medium_lds=0, hmc_traj=1)),
    ((1536, 8, 3, 0), dict(fused=1, fused_lds=163072, nsplit=64, fsplit=6)),
    ((1537, 8, 3, 0), dict(Mp=1600, fused=0, fused_lds=0)),
    ((1025, 20, 513, 0), dict(Mp=1088, nsplit=63, fsplit=4, hmc_traj=0)),
    ((100, 64, 1, 0), dict(DP=64, big=0, nsplit=8)),
    ((100, 65, 1, 0), dict(DP=128, nbk=2, npairs=3)),
    ((300, 40, 130, I8(6)), dict(NB=3, DP=48, Mp=320, nsplit=20, fsplit=1, gpart_planes=0)),
    ((203, 33, 7, I8(5)), dict(NB=3, DP=48, Mp=256, nsplit=16, fsplit=1, gpart_planes=0)),
    ((300, 100, 4, I8(6)), dict(NB=4, DP=128, Mp=320, nsplit=20, fsplit=1, gpart_planes=0)),
    ((10000, 64, 8192, I8(6)), dict(nsplit=4)),
    ((50000, 256, 4096, I8(6)), dict(nsplit=24)),
    ((10000, 64, 128, I8(6)), dict(nsplit=64, fsplit=16, gpart_planes=16)),
    ((30000, 64, 256, I8(6)), dict(nsplit=64, fsplit=8, gpart_planes=8)),
]
# (M, D, n, S): S chunk bn nks NP NPp nkp NRp nCp | ksplit_a ksplit_l tail_pieces (None: no tail accumulator) Gbase
INT8 = {
    "int8": ((300, 40, 130, 6), 6, 682, 128, 10, 820, 896, 26, 384, 256, 1, 3, 8, 0),
    "int8_s5": ((203, 33, 7, 5), 5, 819, 128, 7, 561, 640, 18, 256, 128, 1, 2, 8, 0),
    "large_int8": ((300, 100, 4, 6), 6, 682, 128, 10, 5050, 5120, 158, 384, 128, 1, 1, 8, 1),
    "c3_i8": ((10000, 64, 8192, 6), 6, 682, 128, 313, 2080, 2176, 65, 10112, 8192, 1, 1, 4, 0),
    "c5_i8": ((50000, 256, 4096, 6), 6, 682, 128, 1563, 32896, 32896, 1028, 50048, 4096, 1, 1, None, 1),
    "i8_ksplit": ((10000, 64, 128, 6), 6, 682, 128, 313, 2080, 2176, 65, 10112, 128, 15, 3, None, 0),
    "i8_long": ((30000, 64, 256, 6), 6, 682, 128, 938, 2080, 2176, 65, 30080, 256, 1, 1, 8, 0),
    "i8_s7": ((300, 40, 130, 7), 7, 585, 64, 10, 820, 832, 26, 320, 256, 1, 3, None, 0),
    "i8_s4": ((300, 40, 130, 4), 4, 1023, 128, 10, 820, 896, 26, 384, 256, 1, 3, 8, 0),
}
INT8_KEYS = ("i8S", "i8_chunk", "i8_bn", "i8_nks", "NP", "NPp", "i8_nkp", "i8_NRp", "nCp", "ksplit_a", "ksplit_l")


@pytest.mark.parametrize("name", list(FULL))
def test_plan_table_default_options(name):
    (M, D, n), *want = FULL[name]
    r = P.probe(M, D, n)
    p = r["plan"]
    assert [p[k] for k in FULL_KEYS] == want[:9], (name, p)
    assert (r["amh"]["nt"], r["amh"]["rows"]) == tuple(want[9:]), (name, r["amh"])
    assert p["medium"] == (p["medium_lds"] > 0) and p["fused"] == (p["fused_lds"] > 0)
    assert (p["M"], p["D"], p["n"], p["nblk"], p["i8_requested"]) == (M, D, n, p["Mp"] // 64, 0)


def test_plan_table_single_fields():
    res = P.probe_many(P.probe_line(*shape) for shape, _ in PARTIAL)
    for (shape, want), r in zip(PARTIAL, res):
        assert {k: r["plan"][k] for k in want} == want, (shape, r["plan"])
    assert (lambda a: (a["nt"], a["rows"]))(P.probe(600, 40, 1024)["amh"]) == (64, 10)


@pytest.mark.parametrize("name", list(INT8))
def test_plan_table_int8(name):
    (M, D, n, S), *want = INT8[name]
    p = P.plan(M, D, n, I8(S))
    assert [p[k] for k in INT8_KEYS] == want[:11], (name, p)
    tail_pieces, gbase = want[11:]
    assert p["tail_acc"] == (tail_pieces is not None) and p["gbase"] == gbase and p["i8_requested"] == 1
    if tail_pieces is not None:
        assert p["tail_pieces"] == tail_pieces
    assert p["hpart_at_create"] == 0


def test_plan_table_options():
    c3, c3_i8 = (10000, 64, 8192), (10000, 64, 8192, I8(6))
    assert P.plan(*c3_i8)["tail_acc"] == 1 and P.plan(*c3_i8, i8_tail=0)["tail_acc"] == 0
    assert P.plan(600, 40, 70, fsplit=5)["fsplit"] == 5
    assert P.plan(*c3, nsplit_max=8)["nsplit"] == 4
    assert P.plan(*c3, nsplit_waves=6144)["nsplit"] == 12
    assert P.plan(300, 100, 4, I8(6))["gbase"] == 1 and P.plan(300, 100, 4, I8(6), i8_delta=0)["gbase"] == 0
    assert P.plan(1000, 20, 2048)["hmc_traj"] == 1 and P.plan(1000, 20, 2048, hmc_traj_maxn=100)["hmc_traj"] == 0
    # the fp64 leverage planes of the large-D path: at create without the int8 flag, late (set_data) with it
    assert P.plan(200, 70, 3)["hpart_at_create"] == 1 and P.plan(300, 40, 20)["hpart_at_create"] == 0


def test_int8_assembly_launch_geometry():
    """WN 4, TN 1 (the tile of 4 to 6 slices)"""
    keys = ("WN", "TN", "nCB", "nPB", "nPBfull", "tail", "npb", "nblk_main")
    g = P.probe(10000, 64, 8192, I8(6))["i8"]
    assert [g[k] for k in keys] == [4, 1, 64, 17, 16, 1, 16, 1024] and (g["pb32_0"], g["ntail"]) == (64, 1)
    assert g["k_pieces"] == [dict(ks0=0, nk=313, tail_pieces=4)]
    g = P.probe(300, 40, 130, I8(6))["i8"]
    assert [g[k] for k in keys] == [4, 1, 2, 7, 6, 0, 7, 14]
    g = P.probe(300, 40, 130, I8(6), options=dict(i8_tail=1))["i8"]
    assert [g[k] for k in keys] == [4, 1, 2, 7, 6, 1, 6, 12] and (g["pb32_0"], g["ntail"]) == (24, 2)
    assert g["k_pieces"] == [dict(ks0=0, nk=10, tail_pieces=1)]
    # nks > chunk: two k pieces at launch
    g = P.probe(30000, 64, 256, I8(6))["i8"]
    assert [(k["ks0"], k["nk"]) for k in g["k_pieces"]] == [(0, 682), (682, 256)]
    g = P.probe(300, 40, 130, I8(7))["i8"]
    assert (g["WN"], g["TN"], g["tail"]) == (2, 1, 0)


GRID_M = (1, 63, 64, 65, 1000, 10000, 50000)
GRID_D = (1, 8, 9, 16, 17, 32, 33, 64, 65, 128, 256)
GRID_N = (1, 15, 16, 127, 128, 511, 512, 513, 1023, 1024, 8192)


def grid_lines():
    return [P.probe_line(M, D, n, fl) for M in GRID_M for D in GRID_D for n in GRID_N for fl in (0, I8(6))]


def test_plan_invariants_over_the_grid():
    res = P.probe_many(grid_lines())
    assert len(res) == 7 * 11 * 11 * 2
    for r in res:
        assert r["check"]["code"] == 0 and r["option_error"] is None, r
        p = r["plan"]
        what = (p["M"], p["D"], p["n"], p["i8_requested"])
        assert 1 <= p["nsplit"] <= min(64, p["Mp"] // 16), what                  # (nsplit_max = 64 by default)
        if p["D"] > 64 or p["n"] >= 1024:
            assert p["fsplit"] == 1, what
        assert p["gpart_planes"] in (0, max(p["fsplit"], p["ksplit_a"])), what
        if p["D"] > 64:
            assert p["ksplit_a"] == p["ksplit_l"] == 1, what
        if p["tail_acc"]:
            assert p["ksplit_a"] == 1 and p["i8_bn"] == 128 and p["NP"] % 128 != 0, what
        assert not (p["fused"] and p["medium"]), what
        if p["i8_requested"]:
            g = r["i8"]
            bn = 32 * g["TN"] * g["WN"]
            assert g["nblk_main"] == (g["nCB"] if g["nCB"] < 8 else (g["nCB"] + 7) // 8 * 8) * g["npb"], what
            covered = g["npb"] * bn + (32 * g["ntail"] if g["tail"] else 0)
            assert covered == ((p["NP"] + 31) // 32 * 32 if g["tail"] else p["NPp"]), what
        else:
            assert "i8" not in r and p["i8S"] == 0 and p["nCp"] == 0, what


MSG_D = "rmhmc_create: D > 256 is not supported (64 < D <= 256 uses the blocked large-D path)"
MSG_4GB = "rmhmc_create: the data matrix of the D <= 64 path must stay below 4 GB"
MSG_BIG = "rmhmc_create: M or n_chains too large"


def test_plan_check():
    """every rejection of test_shape_limits_rejected_before_any_device_call (tests/test_capi_library.py) with its message, the other
    argument checks of rmhmc_create, and an accepted shape on either side of each limit"""
    UNSUPPORTED, INVALID = -4, -1
    refused = [((100, 257, 1), UNSUPPORTED, MSG_D), (((1 << 23) + 1, 64, 1), UNSUPPORTED, MSG_4GB), ((1 << 25, 16, 1), UNSUPPORTED, MSG_4GB),
               (((1 << 23) - 63, 64, 1), UNSUPPORTED, MSG_4GB), (((1 << 25) - 63, 16, 1), UNSUPPORTED, MSG_4GB),
               (((1 << 30) + 1, 65, 1), UNSUPPORTED, MSG_BIG), ((10, 3, (1 << 30) + 1), UNSUPPORTED, MSG_BIG),
               ((0, 3, 1), INVALID, "rmhmc_create: bad shape"), ((10, 0, 1), INVALID, "rmhmc_create: bad shape"),
               ((10, 3, 0), INVALID, "rmhmc_create: bad shape")]
    for shape, code, msg in refused:
        assert P.probe(*shape)["check"] == dict(code=code, msg=msg), shape
    assert P.probe(10, 3, 1, dtype=1)["check"] == dict(code=UNSUPPORTED, msg="rmhmc_create: only float64 is built (the reference is float64)")
    assert P.probe(10, 3, 1, _capi.FLAG_ORACLE_LITERAL)["check"] == dict(code=UNSUPPORTED,
                                                                        msg="rmhmc_create: the literal variant exists only in the CPU oracle")
    for shape in ((100, 256, 1), ((1 << 23) - 64, 64, 1), ((1 << 25) - 64, 16, 1), (1 << 30, 65, 1), (10, 3, 1 << 30)):
        r = P.probe(*shape)
        assert r["check"] == dict(code=0, msg="") and (r["plan"]["M"], r["plan"]["D"], r["plan"]["n"]) == shape, shape


def test_options_refused_as_on_the_device():
    """test_gpu_parity.py: create-time keys are refused by rmhmc_set_option, unknown keys and values out of range always"""
    err = lambda **kw: P.probe(300, 40, 20, **kw)["option_error"]
    for key, val, why in (("ccache", 0, "create_only"), ("no_such_option", 1, "unknown"), ("graph", 2, "range")):
        assert err(set_options={key: val}) == dict(key=key, why=why, at="set")
    assert err(options={"no_such_option": 1}) == dict(key="no_such_option", why="unknown", at="create")
    assert err(options={"graph": 2}) == dict(key="graph", why="range", at="create")
    for key, lo, hi in (("fsplit", 0, 64), ("nsplit_max", 1, 1 << 20), ("i8_tail", -1, 1), ("hmc_traj_maxn", -1, 1 << 40)):
        assert err(options={key: lo}) is None and err(options={key: hi}) is None
        assert err(options={key: lo - 1})["why"] == "range" and err(options={key: hi + 1})["why"] == "range"
    for key in ("graph", "sorted", "inflight", "cdyn", "crestore", "i8_force_rebase"):           # the run-time options
        assert err(set_options={key: 1}) is None
    for key in ("medium", "fused", "hmc_traj_maxn", "fsplit", "nsplit_max", "nsplit_waves", "i8_tail", "i8_delta", "i8_delta_inner"):
        assert err(set_options={key: 1})["why"] == "create_only"
