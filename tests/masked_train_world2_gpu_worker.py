"""Child process of tests/test_masked_train_gpu.py::test_two_ranks_over_gloo: rank RANK of a world_size-2 `gloo` group on the
one GPU.  Each rank runs 3 masked BSC EM steps on its ragged `rank::2` shard; the ranks' parameters are gathered
and must be bitwise identical, and within the step tolerance of the NumPy reference whose statistics are formed per shard
and added, and of a one-rank run on the concatenated shards.  Prints "ok <rank>" on success."""
import datetime
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch
import torch.distributed as dist

import masked_train_reference as T

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
    D, H, Hp, g, N = 24, 10, 5, 3, 301
    rng = np.random.RandomState(3)
    params, Y, M = T.model_problem(rng, D, H, N)
    Yh = np.where(M, Y, np.nan)
    an = T.Anneal(T=1.1)
    shards = [np.arange(N)[r::world] for r in range(world)]
    order = np.concatenate(shards)
    m = BSC_ET(D, H, Hp, g, comm=comm)
    p, pr = dict(params), dict(params)
    for _ in range(3):
        p = m.step(an, dict(p), {"y": Yh[shards[rank]], "mask": M[shards[rank]]})
        pr, rlog = T.step(an, pr, Yh, M, Hp, g, shards=shards)
    flat = np.concatenate([np.asarray(p["W"]).ravel(), [p["pi"], p["sigma"]]])
    gathered = comm.allgather(flat.tobytes())
    assert all(b == gathered[0] for b in gathered), "the ranks' parameters differ"
    errs = (rel(p["W"], pr["W"]), abs(p["pi"] / pr["pi"] - 1), abs(p["sigma"] / pr["sigma"] - 1))
    print("rank %d: against the sharded NumPy reference W %.2e pi %.2e sigma %.2e, kept %d" % ((rank,) + errs + (m.W_kept,)))
    assert max(errs) <= RTOL_STEP and m.W_kept == rlog["W_kept"] == 1
    dist.barrier()
    dist.destroy_process_group()
    # the one-rank run on the concatenated shards (no group any more: a solo communicator)
    one = BSC_ET(D, H, Hp, g, comm=parallel.Comm())
    q = dict(params)
    for _ in range(3):
        q = one.step(an, dict(q), {"y": Yh[order], "mask": M[order]})
    errs = (rel(p["W"], q["W"]), abs(p["pi"] / q["pi"] - 1), abs(p["sigma"] / q["sigma"] - 1))
    print("rank %d: against the one-rank run W %.2e pi %.2e sigma %.2e" % ((rank,) + errs))
    assert max(errs) <= RTOL_STEP
    print("ok %d" % rank)


if __name__ == "__main__":
    main()
