"""The inputs of the block-size and edge tests of tests/test_gpu_{gibbs,iwls,amh}.py (tests/helpers/sampler_edges.py), checked on the
NumPy restatements alone: every condition that makes a case fit to carry its bound on the device - the restatement's own stability, the
m/s bins the truncated-normal batch reaches, the capped row, the decision margins of IWLS, saturation in chain 32, the kernel variant
each AMH shape selects - so that a badly chosen input shows here, without a GPU."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import plan_probe  # noqa: E402
import sampler_edges as E  # noqa: E402


# ---- Gibbs ------------------------------------------------------------------------------------------------------------------------------
def test_gibbs_edge_cases_cover_every_block_count_and_row_edge():
    D = {d for _, d, _ in E.GIBBS_EDGE_CASES}
    M = {m for m, _, _ in E.GIBBS_EDGE_CASES}
    assert {(d + 15) // 16 for d in D} >= {1, 2, 3} and {1, 16, 32, 48} <= D        # (NB = 4 and D = 64: test_sample_matches_numpy_philox_d64)
    assert sum(17 <= d <= 32 for d in D) >= 3
    assert {16, 17, 256, 257} <= M and min(M) < 8 and any(8 < m < 16 for m in M)


@pytest.mark.parametrize("M,D,T", E.GIBBS_EDGE_CASES)
def test_gibbs_edge_case_is_stable_on_the_restatement(M, D, T):
    """the criterion of DESIGN section 8d: beta moves by <= 1e-10 when the initial uniforms move one ulp; both labels, no capped row"""
    k = E.gibbs_edge_case(M, D, T)
    print("M %d D %d: the restatement against itself one ulp off: %.3e" % (M, D, k["own"]))
    assert k["own"] <= 1e-10, k["own"]
    tt = np.asarray(k["t"]).reshape(-1)
    assert (tt == 1).any() and (tt == 0).any()
    assert np.all(k["ref"]["capped"] == 0) and np.all(np.isfinite(k["ref"]["beta"]))


def _bin_counts(a):
    b = E.tn_bin_of(a)
    return [int((b == i).sum()) for i in range(len(E.TN_BINS))]


def test_truncated_normal_batch_reaches_every_bin():
    """Over the three iterations every m/s bin between the tapes' range and the tail form is drawn from, both sides of the switch at 25
    included, and large negative m/s; no capped row; no element of Z moves by more than 1e-11 relative with the initial uniforms one
    ulp off.
    The chains relax within one iteration (m/s of the label-1 rows falls to a fifth of z0 in the second sweep), so everything beyond
    m/s = 10 is drawn in the FIRST sweep, and Z after three iterations holds none of those draws.  The one-iteration run of the same
    batch is therefore held to the same counts on the draws its Z consists of: that run is where the device's values are compared
    element by element in every bin."""
    for T in (E.TN_T, 1):
        k = E.tn_mid_case(T)
        ref = k["ref"]
        calls, last = _bin_counts(ref["a_calls"]), _bin_counts(ref["m_last"] / ref["s_last"])
        print("T = %d: draws per m/s bin over all sweeps %s; of the last sweep (the elements of Z) %s; stability %.2e, extreme elements "
              "%.2e of their tolerance" % (T, dict(zip([b[:2] for b in E.TN_BINS], calls)), last, k["own"], k["own_extreme"]))
        counted = calls if T > 1 else last
        for (lo, hi, need), got in zip(E.TN_BINS, counted):
            assert got >= need, (T, lo, hi, got)
        a = ref["a_calls"] if T > 1 else ref["m_last"] / ref["s_last"]
        assert (a < E.TN_BELOW).sum() >= E.TN_BELOW_MIN
        assert np.all(ref["capped"] == 0) and np.all(k["plain_capped"] == 0)
        assert k["own"] <= 1e-11, k["own"]
        # (where U is the last double below 1 the draw is the rounding of m + s y: stable in units of the tolerance, not relatively)
        assert k["own_extreme"] <= 0.01, k["own_extreme"]
    # the one-iteration run is the first sweep of the other (chains with an extreme uniform apart: it sits in another sweep)
    one, three = E.tn_mid_case(1)["ref"], E.tn_mid_case(E.TN_T)["ref"]
    same = [c for c in range(len(E.TN_Z0)) if c not in E.TN_EXTREME_U]
    np.testing.assert_array_equal(one["a_calls"][same], three["a_calls"][same, :E.TN_M])


def test_truncated_normal_extreme_uniforms_stay_on_their_side():
    """1e-300, 2^-53, 1/2 and 1 - 2^-53 on two rows of each label in two chains (and both ends in the tail form of a third): finite,
    non-zero, on the label's side.  BOTH clamps of truncnorm_neg are reached: fmin(x, -TINY) where the mirrored uniform is 1 (Z is
    -TINY), and fmax(p, TINY) on the two label-0 rows drawn at a subnormal uniform (p = U Phi(-m/s) < TINY on the two-tail form:
    the draw is m + s Phi^-1(TINY), about m - 37.5 s)"""
    clamped = 0
    for T in (E.TN_T, 1):
        k = E.tn_mid_case(T)
        ext, Z = k["extreme"], k["ref"]["Z"]
        lab1 = (np.asarray(k["t"]).reshape(-1) == 1)[None] & ext
        for c in E.TN_EXTREME_CHAINS:
            assert sorted(E.TN_EXTREME_U[c].values()) == [1e-300, 2.0 ** -53, 0.5, E.U_MAX]
            assert lab1[c].sum() == 2 and (ext[c] & ~lab1[c]).sum() == 2
        assert np.all(np.isfinite(Z[ext])) and np.all(Z[ext] != 0)
        assert np.all(Z[lab1] > 0) and np.all(Z[ext & ~lab1] < 0)
        clamped += int(np.sum(np.abs(Z[ext]) == E.G.TINY))
        # the fmax(p, TINY) clamp: p below TINY on the two-tail form, on exactly the subnormal uniforms, and the draw is the clamped one
        ref = k["ref"]
        low = ref["p_last"] < E.G.TINY                                         # (NaN, the tail form, compares false)
        sub = np.zeros(ext.shape, bool)
        for c, rows in E.TN_EXTREME_U.items():
            for j, u in rows.items():
                sub[c, j] = u < E.G.TINY
        assert sub.sum() == 2 and np.array_equal(low, sub) and not np.any(sub & lab1)
        want = ref["m_last"][sub] + ref["s_last"][sub] * E.G._ndtri(E.G.TINY)
        np.testing.assert_array_equal(Z[sub], want)
        assert np.all(Z[sub] < ref["m_last"][sub] - 37 * ref["s_last"][sub])
    assert clamped >= 1
    a = E.tn_mid_case(1)["ref"]["m_last"] / E.tn_mid_case(1)["ref"]["s_last"]
    assert np.any(a[ext] > E.G.TAIL) and np.any(a[ext] < 0)


def test_far_tail_batch_is_drawn_beyond_the_switch():
    """at least 20 draws beyond m/s = 25, all of them in the first sweep: the one-iteration run has them in its Z"""
    for T in (E.TN_T, 1):
        ref = E.tn_far_case(T)["ref"]
        assert (ref["a_calls"] > E.G.TAIL).sum() >= 20 and np.all(ref["capped"] == 0)
    ref = E.tn_far_case(1)["ref"]
    assert (ref["m_last"] / ref["s_last"] > E.G.TAIL).sum() >= 20


def test_capped_row_on_the_restatement():
    """one row whose every attempt is rejected: 64 attempts, one capped row in its chain, everything finite, the other chains as on the
    plain streams bit for bit"""
    k = E.capped_case()
    ref, plain = k["ref"], k["plain"]
    np.testing.assert_array_equal(ref["capped"], [0, 1, 0])
    att = ref["attempts"]
    assert att[E.CAP_CHAIN, E.CAP_IT, E.CAP_ROW] == E.G.MAX_ATTEMPTS
    rest = np.ones(att.shape, bool)
    rest[E.CAP_CHAIN, E.CAP_IT, E.CAP_ROW] = False
    assert att[rest].max() < E.G.MAX_ATTEMPTS // 2
    assert E.CAP_IT < E.CAP_T - 1                                  # an iteration follows on the proposal the row kept
    for key in ("beta", "B", "Z", "lam"):
        assert np.all(np.isfinite(ref[key])), key
        for c in (0, 2):
            np.testing.assert_array_equal(ref[key][c], plain[key][c])
    assert np.all(ref["lam"] > 0) and not np.array_equal(ref["beta"][1], plain["beta"][1])
    np.testing.assert_array_equal(ref["beta"][1, :E.CAP_IT + 1], plain["beta"][1, :E.CAP_IT + 1])


# ---- IWLS -------------------------------------------------------------------------------------------------------------------------------
def test_iwls_edge_cases_cover_the_block_counts():
    D = {c[1] for c in E.IWLS_EDGE_CASES}
    assert {(d + 15) // 16 for d in D} >= {1, 2, 3} and {1, 16, 48} <= D and sum(33 <= d <= 48 for d in D) >= 3
    assert any(c[2] == 33 for c in E.IWLS_EDGE_CASES)


@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("case", E.IWLS_EDGE_CASES)
def test_iwls_edge_case_decisions_are_clear_of_their_thresholds(case, compat):
    """no ratio within 1e-6 of 0, none within 1e-6 of log u where u is read; proposals are accepted and rejected"""
    ref = E.iwls_edge_case(case, compat)["ref"]
    m0, mu = E.iwls_margins(ref)
    rate = ref["accepted"].mean()
    print(case, compat, "min |ratio| %.2e, min |ratio - log u| %.2e, acceptance %.2f" % (m0, mu, rate))
    assert m0 >= E.IWLS_MARGIN and mu >= E.IWLS_MARGIN
    assert 0.05 <= rate <= 0.95 and np.all(np.isfinite(ref["w"]))


def test_iwls_chain_32_saturates_on_australian():
    ref = E.iwls_sat_case()["ref"]
    per_chain = ref["saturated"].sum(axis=1)
    print("saturated proposals per chain:", per_chain)
    assert per_chain.shape == (33,) and per_chain[32] >= 1 and per_chain[:32].min() >= 1
    m0, mu = E.iwls_margins(ref)
    assert m0 >= E.IWLS_MARGIN and mu >= E.IWLS_MARGIN
    assert ref["accepted"].any(axis=1).all()


# ---- AMH --------------------------------------------------------------------------------------------------------------------------------
def test_amh_edge_cases_select_the_variants_they_are_named_for():
    """amh_shape of the host (csrc/plan.h, asked through the probe) and AMH_SWITCH of the device header: NT, R as the table says; D > 128
    at NT 64, D > 64 at NT 256, D = 256, an odd D above 64, and the four edges of M"""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "riemannhamiltonianmontecarlo_amd", "csrc")
    plan_h, dev = open(os.path.join(csrc, "plan.h")).read(), open(os.path.join(csrc, "amh.hip.h")).read()
    assert "#define AMH_MAX_ONCHIP_ROWS (256 * 48)" in plan_h
    switch = dev[dev.index("#define AMH_SWITCH("):]
    switch = switch[:switch.index("while (0)")]
    variants = [(int(nt), int(r)) for nt, r in re.findall(r"NT_ = (\d+), R_ = (\d+)", switch)]
    assert variants == [(64, 4), (64, 8), (64, 16), (256, 0), (256, 2), (256, 4), (256, 8), (256, 16), (256, 32), (256, 48)]
    assert re.findall(r"\(R\) (<=|==) (\d+)", switch) == [("<=", "4"), ("<=", "8"), ("==", "0"), ("<=", "2"), ("<=", "4"), ("<=", "8"),
                                                          ("<=", "16"), ("<=", "32")]

    def instantiated(shape):
        """(NT, R) of the variant AMH_SWITCH runs for the host's (NT, rows per thread): the smallest R_ that holds the rows"""
        nt, rows = shape["nt"], shape["rows"]
        return nt, (0 if rows == 0 else min(r for v, r in variants if v == nt and rows <= r))

    cases = E.AMH_EDGE_CASES
    edges = [(1024, 1024), (1024, 1025), (3, 12288), (3, 12289)]
    res = plan_probe.probe_many([plan_probe.probe_line(M, D, n) for n, M, D, *_ in cases.values()]
                                + [plan_probe.probe_line(M, 4, n) for n, M in edges])
    shapes = [instantiated(r["amh"]) for r in res]
    for (name, (n, M, D, T, B, seed, shape)), got in zip(cases.items(), shapes):
        assert got == shape, name
        assert 0 < B < T <= 10 and D <= 256
    assert any(s[6][0] == 64 and s[2] == 256 for s in cases.values())
    assert any(s[6][0] == 64 and s[2] > 128 and s[2] % 2 == 1 for s in cases.values())
    assert sum(s[6][0] == 256 and s[2] > 64 for s in cases.values()) >= 2
    assert {1024, 1025, 12288, 12289} <= {s[1] for s in cases.values()}
    e = shapes[len(cases):]
    assert e[0] == (64, 16) and e[1][0] == 256
    assert e[2] == (256, 48) and e[3] == (256, 0)


@pytest.mark.parametrize("name", list(E.AMH_EDGE_CASES))
def test_amh_edge_case_accepts_and_rejects(name):
    k = E.amh_edge_case(name)
    ref, n = k["ref"], E.AMH_EDGE_CASES[name][0]
    assert len(k["ids"]) == (n if n <= 64 else 18) and k["ids"][0] == 0 and k["ids"][-1] == n - 1
    rate = ref["accepted"].mean()
    assert 0.05 <= rate <= 0.95 and np.all(np.isfinite(ref["w"])) and np.all(np.isfinite(ref["ljl"]))
    assert len(np.unique(ref["sd"])) >= 2                         # the adaptation of iteration 0 moved the proposal SDs both ways
