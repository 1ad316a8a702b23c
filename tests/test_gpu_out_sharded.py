"""multi_gpu.sample_sharded(sampler=...) for all six samplers: three gloo ranks on the one GPU (5 chains in shards of 2 / 2 / 1), one
launch for everything, against single-process calls.  The Philox keys are global chain ids and none of these shapes crosses a path
threshold, so samples, counters and the device statistics are equal bit for bit.  Needs an MI355X: run with  pytest -m gpu."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, synthetic_logreg
from riemannhamiltonianmontecarlo_amd import _capi, experiment
from riemannhamiltonianmontecarlo_amd.multi_gpu import _SHARDED

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import out_ref as R  # noqa: E402
import sharded_out_child as child  # noqa: E402

pytestmark = pytest.mark.gpu


def test_every_sampler_sharded_under_gloo(hip, tmp_path):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = str(tmp_path / "r0.npz")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc_per_node=3", "--master_addr=127.0.0.1",
           "--master_port=%d" % port, os.path.join(ROOT, "tests", "helpers", "sharded_out_child.py"), out]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-4000:]
    g = np.load(out)
    XX, t = synthetic_logreg(child.M, child.D, 3)
    for name in experiment.SAMPLERS:
        key = _SHARDED[name][0]
        counters = [k for k, _ in _capi.SAMPLERS_TO[key][1]]
        with hip.context(child.M, child.D, child.N_CHAINS, flags=_capi.COMPAT if name == "RMHMC" else 0) as ctx, np.errstate(all="ignore"):
            ctx.set_data(XX, t)
            one = R.existing_call(ctx, key, child.N_ITER, child.BURN, seed=child.SEED)
            st = getattr(ctx, "sample_stats" if key == "rmhmc" else key + "_sample_stats")(child.N_ITER, child.BURN, seed=child.SEED)
        assert np.array_equal(g[name + ".samples"], one["samples"]), name
        for k in counters:
            for gather in ("samples", "summary"):
                assert np.array_equal(g["%s.%s.%s" % (name, gather, k)], one[k]), (name, gather, k)
            assert np.array_equal(st[k], one[k]), (name, k)
        assert np.array_equal(g[name + ".mean"], st["mean"]) and np.array_equal(g[name + ".var"], st["var"]), name
        assert np.array_equal(g[name + ".min_ess"], st["ess"].min(1)) and np.isfinite(st["ess"]).all(), name
