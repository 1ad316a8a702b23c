"""Child of tests/test_gpu_out_sharded.py, one rank of three under torch.distributed.run (gloo, all on GPU 0): every sampler of
experiment.SAMPLERS through multi_gpu.sample_sharded in both gather modes, 5 chains in shards of 2 / 2 / 1; rank 0 writes what it
gathered to the .npz named on the command line."""
import os
import sys

import numpy as np
import torch  # noqa: F401  (before the HIP library is loaded: one HIP runtime per process)
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from riemannhamiltonianmontecarlo_amd import experiment  # noqa: E402
from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg  # noqa: E402
from riemannhamiltonianmontecarlo_amd.multi_gpu import sample_sharded  # noqa: E402

M, D, N_CHAINS, N_ITER, BURN, SEED = 200, 5, 5, 40, 15, 21


def main(outfile):
    os.environ["LOCAL_RANK"] = "0"   # three ranks on the one GPU
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    XX, t = synthetic_logreg(M, D, 3)
    if rank != 0:
        XX = t = None                # broadcast from rank 0
    out = {}
    for name in experiment.SAMPLERS:
        for gather in ("samples", "summary"):
            with np.errstate(all="ignore"):
                r = sample_sharded(XX, t, N_CHAINS, NumOfIterations=N_ITER, BurnIn=BURN, seed=SEED, gather=gather, sampler=name)
            if rank != 0:
                assert r is None
                continue
            payload, secs, info = r
            assert secs > 0 and info["world"] == 3 and info["counts"] == [2, 2, 1]
            if gather == "samples":
                out["%s.samples" % name] = payload
            else:
                for k, v in payload.items():
                    out["%s.%s" % (name, k)] = v
            for k, v in info.items():
                if k not in ("world", "counts"):
                    out["%s.%s.%s" % (name, gather, k)] = v
    if rank == 0:
        np.savez(outfile, **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
