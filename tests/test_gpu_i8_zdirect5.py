"""The ZDIRECT form of the 5-slice int8 tile (option i8_zdirect, bit 1; csrc/metric_i8.hip.h: gemm_i8_tile_zd at S = 5) against the LDS
form of the same binary.  The 5-slice tile is the assembly and the leverage pass of a 5-slice context, and at 6 slices the first position
iterate (both inner iterates with i8_delta_inner = 0), the leverage pass and the S' = 5 branch of the delta assemblies.  Both forms sum
the same integers and share the epilogue: every comparison below is BITWISE between two contexts that differ in i8_zdirect only, 1 (the
4-slice tiles alone) against 3 (the 4- and the 5-slice tiles).  tests/test_gpu_i8_zdirect.py compares 0 with 1.
Needs an MI355X: run with  pytest -m gpu."""
import os
import sys

import numpy as np
import pytest

from riemannhamiltonianmontecarlo_amd import _capi
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import plan_probe as P  # noqa: E402

pytestmark = pytest.mark.gpu


def _both(hip, M, D, n, XX, t, fn, flags, options=None):
    """fn(ctx) under i8_zdirect = 1 and = 3"""
    out = []
    for zd in (1, 3):
        with hip.context(M, D, n, flags=flags, options=dict(options or {}, i8_zdirect=zd)) as ctx:
            assert ctx.options()["i8_zdirect"] == zd
            ctx.set_data(XX, t, 100.0)
            assert ctx.int8_certificate()[1]   # (the int8 kernels are in use)
            out.append(fn(ctx))
    return out


def _same(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.array_equal(a, b, equal_nan=True), what


# (i8_nks, ksplit_l, chain blocks, tail tiles) of the shape: one and two k-stages (fewer than the ring of three is deep), 5 / 13 / 29;
# M not a multiple of 32; 2 / 1 / 3 / 17 chain blocks (fewer than eight: the tiles are dealt round; more: the XCD order); chain counts
# that are no multiple of 128; ragged last pair blocks (D = 40: 820 pairs, D = 33: 561, D = 48: 1176) and D = 64's 2080 pairs with the
# tail tiles; the leverage pass in 3, 2, 4, 3 planes and in one launch
PLAIN = {(20, 40, 130): (1, 3, 2, 0), (33, 33, 7): (2, 2, 1, 0), (129, 48, 300): (5, 4, 3, 0), (400, 40, 300): (13, 3, 3, 0),
         (900, 64, 2100): (29, 1, 17, 1)}


@pytest.mark.parametrize("M,D,n", list(PLAIN))
def test_plain_five_slice_metric(hip, M, D, n):
    fl = _capi.int8_metric_flags(5)
    r = P.probe(M, D, n, fl)
    plan, g = r["plan"], r["i8"]
    assert (plan["i8S"], plan["ksplit_a"], plan["big"]) == (5, 1, 0) and (g["WN"], g["TN"]) == (4, 1), plan
    assert (plan["i8_nks"], plan["ksplit_l"], g["nCB"], g["tail"]) == PLAIN[(M, D, n)], (plan, g)
    XX, t = synthetic_logreg(M, D, 1)
    rs = np.random.RandomState(M + D)
    w = 0.4 * rs.randn(n, D) / np.sqrt(D); p = rs.randn(n, D)
    a, b = _both(hip, M, D, n, XX, t, lambda c: c.metric(w) + c.metric_terms(w, p), fl)
    assert np.isfinite(a[0]).all()
    # (the trace term comes from the leverage pass: the same tile on the transposed operands, contraction over the pairs)
    for x, y, what in zip(a, b, ("G", "half log det", "gradient", "trace term", "quadratic term")):
        _same(x, y, what)


@pytest.mark.parametrize("M,D,n", [(2000, 40, 130), (30000, 12, 130)])
def test_k_range_in_pieces(hip, M, D, n):
    """(2000, 40, 130): few tiles, so the k range is cut into 7 planes that are summed afterwards (gridDim.y pieces of 9 stages);
    (30000, 12, 130): 938 stages, more than one launch may sum in int32 at 5 slices (819), so two launches, the second adding."""
    fl = _capi.int8_metric_flags(5)
    plan = P.plan(M, D, n, fl)
    assert plan["i8S"] == 5
    if M == 2000:
        assert plan["ksplit_a"] == 7, plan
    else:
        assert plan["ksplit_a"] == 1 and (plan["i8_nks"], plan["i8_chunk"]) == (938, 819), plan
    XX, t = synthetic_logreg(M, D, 5)
    w = 0.2 * np.random.RandomState(4).randn(n, D) / np.sqrt(D)
    (G0, _, _), (G1, _, _) = _both(hip, M, D, n, XX, t, lambda c: c.metric(w), fl)
    assert np.isfinite(G0).all()
    _same(G0, G1, "G")


def _leapfrog_outputs(w, p, dirs, steps):
    def fn(ctx):
        w1, p1, hld1, st = ctx.leapfrog(w, p, 0.5, dirs, steps, 4)
        counts = ctx.i8_delta_counts()
        return w1, p1, hld1, st, ctx.metric(w1)[0], counts
    return fn


def _same_leapfrog(a, b):
    assert a[5] == b[5]
    for k, what in enumerate(("theta", "p", "half log det", "status", "G")):
        _same(a[k], b[k], what)


@pytest.mark.parametrize("rebase", [0, 1])
@pytest.mark.parametrize("inner", [1, 0])
@pytest.mark.parametrize("M,D,n", [(203, 33, 7), (400, 40, 2432), (900, 64, 2100)])
def test_six_slice_leapfrog(hip, M, D, n, inner, rebase):
    """Three leapfrog steps at 6 slices, where the 5-slice tile is the first position iterate (i8_delta_inner = 0: both inner iterates)
    and the leverage pass.  i8_force_rebase = 1 puts N itself into the planes of the delta assemblies, which then take their S' = 5
    (inner) and S' = 6 branches."""
    fl = _capi.int8_metric_flags(6)
    plan = P.plan(M, D, n, fl, i8_delta_inner=inner)
    assert (plan["i8S"], plan["big"], plan["ksplit_a"]) == (6, 0, 1), plan
    XX, t = synthetic_logreg(M, D, 5)
    rs = np.random.RandomState(M + n)
    w = 0.4 * rs.randn(n, D) / np.sqrt(D); p = rs.randn(n, D)
    dirs = np.where(rs.rand(n) < 0.5, -1, 1).astype(np.int32)
    a, b = _both(hip, M, D, n, XX, t, _leapfrog_outputs(w, p, dirs, 3), fl,
                 options={"i8_delta": 1, "i8_delta_inner": inner, "i8_force_rebase": rebase})
    print("delta assemblies by slice count:", a[5], b[5])
    if not inner:
        assert sum(a[5]["inner"]) == 0   # (no inner delta assembly: full 5-slice assemblies instead)
    elif rebase:
        assert a[5]["inner"][1] > 0      # (the S' = 5 branch of k_assemble_i8_sel really ran)
    _same_leapfrog(a, b)


@pytest.mark.parametrize("M,D,n", [(400, 80, 130), (96, 256, 130)])
def test_large_d_path(hip, M, D, n):
    """64 < D <= 256, 6 slices, one leapfrog step.  (96, 256, 130): 1028 pair stages against the 682-stage chunk, so the leverage GEMM
    accumulates over two launches."""
    fl = _capi.int8_metric_flags(6)
    plan = P.plan(M, D, n, fl)
    assert (plan["i8S"], plan["big"]) == (6, 1), plan
    if D == 256:
        assert (plan["i8_nkp"], plan["i8_chunk"]) == (1028, 682), plan
    XX, t = synthetic_logreg(M, D, 5)
    rs = np.random.RandomState(M + n)
    w = 0.4 * rs.randn(n, D) / np.sqrt(D); p = rs.randn(n, D)
    dirs = np.where(rs.rand(n) < 0.5, -1, 1).astype(np.int32)
    a, b = _both(hip, M, D, n, XX, t, _leapfrog_outputs(w, p, dirs, 1), fl)
    _same_leapfrog(a, b)


def test_nonfinite_chain_among_finite_ones(hip):
    """A NaN position makes v non-finite: that chain's G comes out NaN and it is rejected, the 139 other chains stay bit-identical to
    a run without it - in both settings, which agree with each other."""
    M, D, n = 400, 40, 140
    XX, t = synthetic_logreg(M, D, 6)
    rs = np.random.RandomState(2)
    w = 0.05 * rs.randn(n, D); z = rs.randn(n, D)
    ul = rs.rand(n); gd = rs.randn(n); ua = rs.rand(n)
    wbad = w.copy(); wbad[17, 3] = np.nan
    keep = np.arange(n) != 17
    # the plain 5-slice assembly
    fl = _capi.int8_metric_flags(5)
    good0, good1 = _both(hip, M, D, n, XX, t, lambda c: c.metric(w)[0], fl)
    bad0, bad1 = _both(hip, M, D, n, XX, t, lambda c: c.metric(wbad)[0], fl)
    for good, bad in ((good0, bad0), (good1, bad1)):
        assert np.isnan(bad[17]).all() and np.isfinite(good).all()
        _same(bad[keep], good[keep], "G of the finite chains")
    _same(good0, good1, "G"); _same(bad0, bad1, "G with the NaN chain")
    # whole transitions at 6 slices (5-slice first iterate and leverage pass)
    fl = _capi.int8_metric_flags(6)
    good0, good1 = _both(hip, M, D, n, XX, t, lambda c: c.transition(w, z, ul, gd, ua, L=3, eps=0.5, K=4), fl)
    bad0, bad1 = _both(hip, M, D, n, XX, t, lambda c: c.transition(wbad, z, ul, gd, ua, L=3, eps=0.5, K=4), fl)
    for good, bad in ((good0, bad0), (good1, bad1)):
        assert bad["accepted"][17] == 0 and bad["status"][17] != 0
        for k in ("w", "w_prop", "H_prop", "accepted"):
            _same(bad[k][keep], good[k][keep], k)
    for k in ("w", "w_prop", "p_prop", "H_prop", "hld_prop", "accepted", "status"):
        _same(good0[k], good1[k], k); _same(bad0[k], bad1[k], k + " with the NaN chain")
