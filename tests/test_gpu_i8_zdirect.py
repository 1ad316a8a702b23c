"""The ZDIRECT form of the 4-slice int8 tile (option i8_zdirect, csrc/metric_i8.hip.h: the Z fragments come straight from global memory
into registers, LDS carries the V part alone) against the LDS form of the same binary.  Both forms sum the same integers, in another
association, and share the epilogue: every comparison below is BITWISE between two contexts that differ in i8_zdirect only.
(That either form is right is the business of tests/test_gpu_int8_metric.py, which runs at the default i8_zdirect = 1.)
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
    """fn(ctx) under i8_zdirect = 0 and = 1"""
    out = []
    for zd in (0, 1):
        with hip.context(M, D, n, flags=flags, options=dict(options or {}, i8_zdirect=zd)) as ctx:
            assert ctx.options()["i8_zdirect"] == zd
            ctx.set_data(XX, t, 100.0)
            assert ctx.int8_certificate()[1]   # (the int8 kernels are in use)
            out.append(fn(ctx))
    return out


def _same(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.array_equal(a, b, equal_nan=True), what


# one, two and five k-stages (fewer than either ring is deep) and 13 / 29; M not a multiple of 32; 2 / 1 / 3 / 17 chain blocks
# (fewer than eight: the tiles are dealt round; more: the XCD order); chain counts that are no multiple of 128; ragged last pair
# blocks (D = 40: 820 pairs, D = 33: 561, D = 48: 1176) and D = 64's 2080 pairs with the tail tiles
@pytest.mark.parametrize("M,D,n", [(20, 40, 130), (33, 33, 7), (129, 48, 300), (400, 40, 300), (900, 64, 2100)])
def test_plain_four_slice_metric(hip, M, D, n):
    XX, t = synthetic_logreg(M, D, 1)
    rs = np.random.RandomState(M + D)
    w = 0.4 * rs.randn(n, D) / np.sqrt(D); p = rs.randn(n, D)
    a, b = _both(hip, M, D, n, XX, t, lambda c: c.metric(w) + c.metric_terms(w, p), _capi.int8_metric_flags(4))
    assert np.isfinite(a[0]).all()
    # (the trace term comes from the leverage pass: the same tile on the transposed operands, contraction over the pairs)
    for x, y, what in zip(a, b, ("G", "half log det", "gradient", "trace term", "quadratic term")):
        _same(x, y, what)


@pytest.mark.parametrize("M,D,n", [(2000, 40, 130), (40000, 12, 130)])
def test_k_range_in_pieces(hip, M, D, n):
    """(2000, 40, 130): few tiles, so the k range is cut into planes that are summed afterwards (gridDim.y pieces of 9 stages);
    (40000, 12, 130): more rows than one launch may sum in int32 at 4 slices (32736), so two launches in sequence, the second adding."""
    fl = _capi.int8_metric_flags(4)
    plan = P.plan(M, D, n, fl)
    assert (plan["ksplit_a"] > 1) if M == 2000 else (plan["ksplit_a"] == 1 and plan["i8_nks"] > plan["i8_chunk"]), plan
    XX, t = synthetic_logreg(M, D, 5)
    w = 0.2 * np.random.RandomState(4).randn(n, D) / np.sqrt(D)
    (G0, _, _), (G1, _, _) = _both(hip, M, D, n, XX, t, lambda c: c.metric(w), fl)
    assert np.isfinite(G0).all()
    _same(G0, G1, "G")


@pytest.mark.parametrize("rebase", [0, 1])
@pytest.mark.parametrize("M,D,n", [(203, 33, 7), (400, 40, 2432), (900, 64, 2100)])
def test_delta_assemblies(hip, M, D, n, rebase):
    """Three leapfrog steps at 6 slices with both delta assemblies on: their S' = 4 branch is the tile in question (k_assemble_i8_sel).
    i8_force_rebase = 1 puts N itself into the planes, which selects the 5- or 6-slice code of the same kernel: unaffected."""
    XX, t = synthetic_logreg(M, D, 5)
    rs = np.random.RandomState(M + n)
    w = 0.4 * rs.randn(n, D) / np.sqrt(D); p = rs.randn(n, D)
    dirs = np.where(rs.rand(n) < 0.5, -1, 1).astype(np.int32)

    def fn(ctx):
        w1, p1, hld1, st = ctx.leapfrog(w, p, 0.5, dirs, 3, 4)
        counts = ctx.i8_delta_counts()
        return w1, p1, hld1, st, ctx.metric(w1)[0], counts

    a, b = _both(hip, M, D, n, XX, t, fn, _capi.int8_metric_flags(6),
                 options={"i8_delta": 1, "i8_delta_inner": 1, "i8_force_rebase": rebase})
    print("delta assemblies by slice count:", a[5], b[5])
    assert a[5] == b[5]
    assert a[5]["end"][0] > 0 if not rebase else a[5]["end"][0] + a[5]["inner"][0] == 0   # (the S' = 4 branch really ran / never ran)
    for k, what in enumerate(("theta", "p", "half log det", "status", "G")):
        _same(a[k], b[k], what)


def test_nonfinite_chain_among_finite_ones(hip):
    """A NaN position makes v non-finite: that chain's G comes out NaN and it is rejected, the 127 chains that share its tile stay
    bit-identical to a run without it - in both forms, which agree with each other."""
    M, D, n = 400, 40, 140
    XX, t = synthetic_logreg(M, D, 6)
    rs = np.random.RandomState(2)
    w = 0.05 * rs.randn(n, D); z = rs.randn(n, D)
    ul = rs.rand(n); gd = rs.randn(n); ua = rs.rand(n)
    wbad = w.copy(); wbad[17, 3] = np.nan
    keep = np.arange(n) != 17
    # the plain 4-slice assembly
    fl = _capi.int8_metric_flags(4)
    good0, good1 = _both(hip, M, D, n, XX, t, lambda c: c.metric(w)[0], fl)
    bad0, bad1 = _both(hip, M, D, n, XX, t, lambda c: c.metric(wbad)[0], fl)
    for good, bad in ((good0, bad0), (good1, bad1)):
        assert np.isnan(bad[17]).all() and np.isfinite(good).all()
        _same(bad[keep], good[keep], "G of the finite chains")
    _same(good0, good1, "G"); _same(bad0, bad1, "G with the NaN chain")
    # whole transitions at 6 slices (delta assemblies)
    fl = _capi.int8_metric_flags(6)
    good0, good1 = _both(hip, M, D, n, XX, t, lambda c: c.transition(w, z, ul, gd, ua, L=3, eps=0.5, K=4), fl)
    bad0, bad1 = _both(hip, M, D, n, XX, t, lambda c: c.transition(wbad, z, ul, gd, ua, L=3, eps=0.5, K=4), fl)
    for good, bad in ((good0, bad0), (good1, bad1)):
        assert bad["accepted"][17] == 0 and bad["status"][17] != 0
        for k in ("w", "w_prop", "H_prop", "accepted"):
            _same(bad[k][keep], good[k][keep], k)
    for k in ("w", "w_prop", "p_prop", "H_prop", "hld_prop", "accepted", "status"):
        _same(good0[k], good1[k], k); _same(bad0[k], bad1[k], k + " with the NaN chain")
