"""Option i8_zdirect is a mask (csrc/plan.h): bit 0 the 4-slice int8 tiles in their ZDIRECT form, bit 1 the 5-slice tiles.  Asked of
the compiled rule on the CPU (tests/helpers/plan_probe)."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import plan_probe as P  # noqa: E402

from riemannhamiltonianmontecarlo_amd import _capi  # noqa: E402


def test_i8_zdirect_is_a_create_time_mask_of_two_bits():
    fl = _capi.int8_metric_flags(6)
    err = lambda **kw: P.probe(300, 40, 130, fl, **kw)["option_error"]
    for v in (0, 1, 2, 3):
        assert err(options={"i8_zdirect": v}) is None, v
    for v in (-1, 4):
        assert err(options={"i8_zdirect": v}) == dict(key="i8_zdirect", why="range", at="create"), v
    for v in (0, 3):
        assert err(set_options={"i8_zdirect": v}) == dict(key="i8_zdirect", why="create_only", at="set"), v


def test_i8_zdirect_changes_no_shape():
    """the form of a tile is chosen at launch: the plan is the same under every value"""
    for M, D, n, S in ((300, 40, 130, 5), (10000, 64, 8192, 6), (400, 80, 130, 6)):
        fl = _capi.int8_metric_flags(S)
        plans = [P.plan(M, D, n, fl, i8_zdirect=v) for v in (0, 1, 2, 3)]
        assert all(p == plans[0] for p in plans[1:]), (M, D, n, S)
