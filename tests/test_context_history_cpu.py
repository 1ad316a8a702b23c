"""CPU twin of tests/test_gpu_context_history.py: the same battery and polluters (tests/helpers/context_history.py) against the CPU
oracle.  It pins the oracle's own statelessness, which the GPU file's anchor relies on, and lets the harness run without a GPU.

Left out because the oracle cannot express them: AMH / IWLS / Gibbs (not exported), the run-time options (accepted and ignored, no
option set to read back) and the int8 certificate (always inactive); K = 0 and the ESS length limit are HIP-only refusals."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import context_history as H  # noqa: E402

# the fused, medium and generic shapes of the GPU file (the oracle has one path only; a battery takes it well under a second at these)
CPU_PATHS = {k: H.PATHS[k] for k in ("fused", "medium", "generic")}
CPU_POLLUTERS = ["other_data_larger", "other_data_smaller", "diverged", "other_samplers", "other_run", "failed_calls", "other_params"]
_fresh = {}


def _context(oracle, spec, variant="own"):
    M, D, n, flags, _ = spec
    ctx = oracle.context(M, D, n, flags=flags)
    ctx.set_data(*H.data_of(spec, variant), 100.0)
    return ctx


def fresh(oracle, path):
    """the battery on a fresh context, once per path; never modified afterwards"""
    if path not in _fresh:
        spec = CPU_PATHS[path]
        with _context(oracle, spec) as ctx:
            _fresh[path] = H.battery(ctx, H.make_inputs(spec))
        for v in _fresh[path].values():
            v.setflags(write=False)
    return _fresh[path]


@pytest.mark.parametrize("path", list(CPU_PATHS))
def test_battery_is_deterministic_and_order_independent(oracle, path):
    spec = CPU_PATHS[path]
    want = fresh(oracle, path)
    assert len(want) > 40 and not any(k.startswith(("amh", "iwls", "gibbs")) for k in want)
    with _context(oracle, spec) as ctx:
        H.assert_same_bits(H.battery(ctx, H.make_inputs(spec)), want, path + " second fresh context")
    with _context(oracle, spec) as ctx:
        H.assert_same_bits(H.battery(ctx, H.make_inputs(spec), order="reversed"), want, path + " reversed")


@pytest.mark.parametrize("polluter", CPU_POLLUTERS)
@pytest.mark.parametrize("path", list(CPU_PATHS))
def test_battery_does_not_depend_on_history(oracle, path, polluter):
    spec = CPU_PATHS[path]
    want = fresh(oracle, path)
    inp = H.make_inputs(spec)
    with _context(oracle, spec) as ctx:
        H.POLLUTERS[polluter](ctx, spec, inp)
        H.assert_same_bits(H.battery(ctx, inp), want, "%s after %s" % (path, polluter))
