"""Child of tests/test_gpu_quant.py, one rank of three (gloo, all on GPU 0; rank and rendezvous from the environment):
multi_gpu.sample_sharded(quantiles=PROBS) for HMC (gather="summary") and AMH (gather="samples") with 7 chains (ragged shards of 3 / 2 / 2)
and with 2 chains (one empty shard); rank 0 writes what it gathered to the .npz named on the command line."""
import os
import sys

import numpy as np
import torch  # noqa: F401  (before the HIP library is loaded: one HIP runtime per process)
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

M, D, N_ITER, BURN, SEED = 200, 5, 40, 15, 21
SAMPLERS = (("HMC", "summary"), ("AMH", "samples"))
CHAINS = ((7, [3, 2, 2]), (2, [1, 1, 0]))   # (chains, the shards they fall into)
PROBS = (0.025, 0.5, 0.975)


def main(outfile):
    from riemannhamiltonianmontecarlo_amd.data import synthetic_logreg
    from riemannhamiltonianmontecarlo_amd.multi_gpu import sample_sharded
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    XX, t = synthetic_logreg(M, D, 3)
    out = {}
    for n_chains, counts in CHAINS:
        for name, gather in SAMPLERS:
            with np.errstate(all="ignore"):
                r = sample_sharded(XX, t, n_chains, NumOfIterations=N_ITER, BurnIn=BURN, seed=SEED, gather=gather, sampler=name,
                                   quantiles=PROBS)
            if rank != 0:
                assert r is None
                continue
            payload, secs, info = r
            assert secs > 0 and info["world"] == 3 and info["counts"] == counts
            pre = "%s.%d." % (name, n_chains)
            out[pre + "accepted"] = info["accepted"]
            out[pre + "quantiles"] = info["quantiles"]
            out[pre + "quantile_draws"] = info["quantile_draws"]
            if gather == "samples":
                out[pre + "samples"] = payload
    if rank == 0:
        np.savez(outfile, **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
