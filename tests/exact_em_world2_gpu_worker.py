"""Child process of tests/test_exact_em_gpu.py::test_two_ranks_over_gloo: rank RANK of a world_size-2 `gloo` group on the one
GPU.  Each rank runs 3 exact BSC EM steps on its ragged `rank::2` shard; the ranks' parameters are gathered and
must be bitwise identical, and within the step tolerance of a one-rank run on the concatenated shards.  Prints "ok <rank>" on
success."""
import datetime
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch
import torch.distributed as dist

import exact_em_reference as X

RTOL_STEP = 1e-8


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    from prosper_amd.utils import parallel
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=300))
    comm = parallel.Comm()
    D, H, N = 16, 11, 201
    params, Y = X.problem(np.random.RandomState(3), D, H, N)
    an = X.Anneal(T=1.1)
    shards = [np.arange(N)[r::world] for r in range(world)]
    order = np.concatenate(shards)
    m = BSC_ET(D, H, 3, 2, comm=comm)
    p = dict(params)
    for _ in range(3):
        p = m.exact_step(an, dict(p), {"y": Y[shards[rank]]})
    flat = np.concatenate([np.asarray(p["W"]).ravel(), [p["pi"], p["sigma"]]])
    gathered = comm.allgather(flat.tobytes())
    assert all(b == gathered[0] for b in gathered), "the ranks' parameters differ"
    dist.barrier()
    dist.destroy_process_group()
    # the one-rank run on the concatenated shards (no group any more: a solo communicator)
    one = BSC_ET(D, H, 3, 2, comm=parallel.Comm())
    q = dict(params)
    for _ in range(3):
        q = one.exact_step(an, dict(q), {"y": Y[order]})
    errs = (rel(p["W"], q["W"]), abs(p["pi"] / q["pi"] - 1), abs(p["sigma"] / q["sigma"] - 1))
    print("rank %d: against the one-rank run W %.2e pi %.2e sigma %.2e" % ((rank,) + errs))
    assert max(errs) <= RTOL_STEP
    print("ok %d" % rank)


if __name__ == "__main__":
    main()
