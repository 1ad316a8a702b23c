"""The references and the case table of tests/test_gpu_ess_edges.py held to their own conditions, without a GPU (tests/helpers/ess_edges.py):
ess_ld, the long-double lag-by-lag estimator, against the reference's recorded outputs and the host restatement tools.CalculateESS;
the conditions a case must meet to test what it is there for; the mutation table: every named error of a kernel, planted in the
float64 restatement of k_ess, is told from a right kernel by at least one case; and the CPU oracle over the whole table in both modes.

Run with -s to see the mutation table and the measured errors."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from riemannhamiltonianmontecarlo_amd import _capi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import ess_edges as E  # noqa: E402

MODES = ("linear", "wrap")
FINITE = [c for c in E.CASES if c.gen[0] != "nonfinite"]
HARD_OFFSET = E.HARD_OFFSET


bounds = E.case_bounds


def assert_within(got, case, mode, who):
    ref = E.case_ref(case, mode)
    e, b = E.errors(got, ref), bounds(case, mode)
    assert e["nan"], (who, case.id, mode, "NaN pattern")
    for k in ("ess", "mean", "var"):
        if k in got:
            assert e[k] <= b[k], (who, case.id, mode, k, e[k], b[k])
    return e


# ---- the reference -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ess_ar1", "ess_pima_chain", "ess_s4096"])
def test_ess_ld_reproduces_the_recorded_reference(name):
    """the goldens are outputs of the reference's Python, whose FFT length is the wrapped one: ess_ld in wrap mode, to the 1e-9 of
    tests/test_tools_ess.py; ess_s4096 (S a power of two) is the one where the linear mode is a different number"""
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    x = g["samples"]
    S = x.shape[0]
    assert int(g["maxlag"]) == S - 1
    r = E.ess_ld(x, E.nfft_of(S, "wrap"))
    print("%s: S = %d, rel err %.1e, pairs %s" % (name, S, np.abs(r["ess"] / g["ess"] - 1).max(), r["pairs"]))
    assert np.allclose(r["ess"], g["ess"], rtol=1e-9, atol=0)
    if name == "ess_s4096":
        lin = E.ess_ld(x, 0)["ess"]
        assert (np.abs(lin / g["ess"] - 1) > 1e-3).any()


@pytest.mark.parametrize("mode", MODES)
def test_ess_ld_agrees_with_the_host_restatement(mode):
    """tools.CalculateESS (FFT) and two-pass NumPy on every finite case, in both modes, to the tolerances of the GPU test.  At a mean of
    1e8 standard deviations the host's own error is the measurement the kernel's bound is made of (printed); what is asserted of it is
    only that it is the rounding of the centred values and no more: each is off by up to |mean| 2^-53 = 1.1e-8 sd, a relative error of
    that size in every lag product, so 1e-6 leaves two orders for the 1 / Gamma amplification of the last pair."""
    worst = dict(ess=0.0, mean=0.0, var=0.0)
    for case in FINITE:
        ref = E.case_ref(case, mode)
        e = E.errors(E.host_restatement(E.case_block(case), mode), ref)
        assert e["nan"], case.id
        if case.id == HARD_OFFSET:
            print("%s %s: host restatement against ess_ld: ess %.2e (rel), mean %.2e, var %.2e (units of the project's tolerance)"
                  % (case.id, mode, e["ess"], e["mean"], e["var"]))
            assert e["ess"] < 1e-6
            continue
        for k in worst:
            worst[k] = max(worst[k], e[k])
        assert e["ess"] <= E.ESS_RTOL and e["mean"] <= 1.0 and e["var"] <= 1.0, (case.id, e)
    print("%s: host restatement against ess_ld, worst over the other cases: %r" % (mode, worst))


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------
def test_case_table_conditions():
    ids = set(E.CASE)
    for S in E.SIZES_LINEAR + (E.S_MAX,):
        assert "size-lin-s%d" % S in ids
    for S in E.SIZES_WRAP:
        assert "size-wrap-s%d" % S in ids
    assert sum(np.asarray(E.case_block(c)).nbytes for c in E.CASES) < 8 << 20
    stops = set()
    clamp = False
    for case in E.CASES:
        x = E.case_block(case)
        assert x.shape == (case.n, case.S, case.P) and x.dtype == np.float64
        for mode in MODES:
            r = E.case_ref(case, mode)
            has = np.isfinite(r["ess"])
            # every column that takes part in an ESS comparison is away from a tie of its stopping rule
            assert (r["margin"][has] > E.MARGIN).all(), (case.id, mode, r["margin"].min())
            if case.gen[0] != "nonfinite":
                assert has.all(), (case.id, mode)
        r = E.case_ref(case)
        has = np.isfinite(r["ess"])
        half = case.S // 2
        stops |= {"first" if p == 1 else "never" if p == half else "middle" for p in r["pairs"][has] if half > 1}
        clamp |= bool((r["clamped"][has] > 0).any())
    assert stops == {"first", "middle", "never"} and clamp
    # the cases that are there for one behaviour have it
    assert (E.case_ref(E.CASE["stop-first-pair"])["pairs"] == 1).all()
    assert (E.case_ref(E.CASE["clamp-fires"])["clamped"] > 0).all()
    for S in E.ALT_S:
        for mode in MODES:
            c = E.CASE["alt-%s-s%d" % (mode[:3], S)]
            r = E.case_ref(c)
            if mode == "linear" or S in (2, 3, 129):           # (S = 64 in wrap mode: the wrapped partners have the other sign)
                assert (r["pairs"] == S // 2).all(), (c.id, r["pairs"])
            if mode == "linear":
                assert (r["ess"] == S).all()                   # tau clamped to 1: see the derivation in the GPU test
    big = E.case_ref(E.CASE["size-lin-s20000"])
    assert big["pairs"].max() < 20                             # nothing quadratic at the limit
    x = E.case_block(E.CASE["size-lin-s20000"])
    assert ((x[:, -1] - x.mean(1)) / x[:, :-1].std(1) > 25).all()


def test_wrap_cases_show_the_wrap_or_provably_cannot():
    for S in E.WRAP_REACHED:
        c = E.CASE["size-wrap-s%d" % S]
        w, l = E.case_ref(c, "wrap")["ess"], E.case_ref(c, "linear")["ess"]
        differ = np.abs(w / l - 1) > 1e-3
        print("%s: %d of %d columns differ by more than 1e-3 between the modes (median %.1e)" % (c.id, differ.sum(), differ.size,
                                                                                                 np.median(np.abs(w / l - 1))))
        assert differ.mean() >= 0.5, c.id
    for c in [E.CASE["width-wra-p%d" % P] for P in E.WIDTHS]:
        assert (np.abs(E.case_ref(c, "wrap")["ess"] / E.case_ref(c, "linear")["ess"] - 1) > 1e-3).mean() >= 0.5, c.id
    for S in E.WRAP_NOT_REACHED:
        c = E.CASE["size-wrap-s%d" % S]
        w, l = E.case_ref(c, "wrap"), E.case_ref(c, "linear")
        first_wrapped = E.nfft_of(S, "wrap") - S + 1
        assert (2 * w["pairs"] + 1 < first_wrapped).all()     # the stopping pair included: lags 2 pairs, 2 pairs + 1
        for k in ("ess", "mean", "var"):
            assert np.array_equal(w[k], l[k]), (c.id, k)


# ---- the mutation table ------------------------------------------------------------------------------------------------------------------------
def test_unmutated_restatement_passes_everywhere():
    for case in E.CASES:
        for mode in MODES:
            got = E.block_restatement(E.case_block(case), E.nfft_of(case.S, mode))
            e = assert_within(got, case, mode, "restatement")
            if case.id == HARD_OFFSET:
                print("%s %s: float64 kernel restatement against ess_ld: ess %.2e, mean %.2e, var %.2e" % (case.id, mode, e["ess"], e["mean"], e["var"]))


def _caught(case, mutation):
    """how the case tells the mutated kernel from ess_ld, in the case's own mode: '' if it does not"""
    if mutation == "stop_on_raw_pair" and case.S > E.ALL_PAIRS_S_MAX:
        return ""
    ref = E.case_ref(case)
    got = E.block_restatement(E.case_block(case), E.nfft_of(case.S, case.mode), mutation)
    how = []
    for k in ("ess", "mean", "var"):
        if not np.array_equal(np.isnan(got[k]), np.isnan(ref[k])):
            how.append(k + ":nan")
        elif E.rel_diff(got, ref, k) > 1e-6:
            how.append(k)
    return "+".join(how)


def test_mutation_table():
    table = {}
    for mutation in E.MUTATIONS:
        table[mutation] = [(c.id, h) for c in E.CASES for h in [_caught(c, mutation)] if h]
    print()
    for mutation, hits in table.items():
        if mutation in E.EQUIVALENT:
            print("%-22s changes no output on any input (test_equivalent_mutation_changes_nothing): caught by %d" % (mutation, len(hits)))
            continue
        print("%-22s caught by %2d case(s): %s" % (mutation, len(hits), ", ".join("%s (%s)" % h for h in hits[:6]) + (" ..." if len(hits) > 6 else "")))
    for mutation, hits in table.items():
        if mutation in E.EQUIVALENT:
            continue
        assert hits, "no case tells %s from a right kernel: the table is missing a case" % mutation
    what = {m: {h for _, hs in hits for h in hs.split("+")} for m, hits in table.items()}
    assert "var" in what["var_sample"] and "ess:nan" in what["no_c0_guard"] and "mean:nan" in what["mean_of_inf_column"]
    # the wrap errors are caught on the ESS, and by wrap-mode cases of a power-of-two length
    for m in ("no_wrap", "wrap_off_by_one_low", "wrap_off_by_one_high", "wrap_at_lag0"):
        assert "ess" in what[m] and any(E.CASE[cid].mode == "wrap" for cid, _ in table[m])
    # the errors of one stride are caught at the sizes that put a row there
    assert any(E.CASE[cid].S in (64, 65) for cid, _ in table["drop_row_63"])
    assert any(cid == "size-lin-s20000" for cid, _ in table["drop_last_row"])


def test_equivalent_mutation_changes_nothing():
    """half = (S + 1) / 2: the extra pair of an odd-length series that never stops cannot lift tau above 1 (the helper's docstring).  The
    table holds such series; the mutated restatement equals the right one on every case, bit for bit."""
    odd_never = 0
    for case in E.CASES:
        r = E.case_ref(case)
        odd_never += int(case.S % 2 == 1 and (r["pairs"][np.isfinite(r["ess"])] == case.S // 2).sum())
        x, nfft = E.case_block(case), E.nfft_of(case.S, case.mode)
        a, b = E.block_restatement(x, nfft, "half_rounds_up"), E.block_restatement(x, nfft)
        assert np.array_equal(a["ess"], b["ess"], equal_nan=True), case.id
    assert odd_never >= 10


def test_scaled_cases_scale_exactly():
    """a power of two is exact in every product and sum while nothing overflows or goes subnormal: c0 is about 2^(2k + 10), normal for
    every k of the table, so ess_ld of the float64 inputs - the expected value of the GPU test - is the base's ESS, and the float64
    restatement is bit-identical across the scales"""
    base = E.CASE[E.SCALE_BASE]
    rb, mb = E.case_ref(base), E.block_restatement(E.case_block(base), 0)
    for k in E.SCALES:
        if k == 0:
            continue
        c = E.CASE["scale-2^%d" % k]
        assert np.array_equal(E.case_block(c), E.case_block(base) * 2.0 ** k)
        r, m = E.case_ref(c), E.block_restatement(E.case_block(c), 0)
        assert np.isfinite(r["var"]).all() and (r["var"] > 2.0 ** -1000).all()
        assert np.allclose(r["ess"], rb["ess"], rtol=1e-15, atol=0)
        assert np.array_equal(m["ess"], mb["ess"]) and np.array_equal(m["mean"], mb["mean"] * 2.0 ** k)
        assert np.array_equal(m["var"], mb["var"] * 4.0 ** k)


# ---- the CPU oracle ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_cpu_oracle_runs_the_table(oracle, mode):
    flags = _capi.FLAG_ESS_WRAP if mode == "wrap" else 0
    worst = 0.0
    with oracle.context(10, 2, 1, flags=flags) as ctx:
        for case in E.CASES:
            got = dict(ess=ctx.ess(E.case_block(case)))
            ref = E.case_ref(case, mode)
            assert np.array_equal(np.isnan(got["ess"]), np.isnan(ref["ess"])), (case.id, mode)
            b = bounds(case, mode)["ess"]
            e = E.rel_diff(got, ref, "ess")
            if case.id == HARD_OFFSET:
                print("%s %s: CPU oracle against ess_ld %.2e (bound %.2e)" % (case.id, mode, e, b))
            else:
                worst = max(worst, e)
            assert e <= b, (case.id, mode, e, b)
    print("%s: CPU oracle against ess_ld, worst over the other cases %.2e" % (mode, worst))
