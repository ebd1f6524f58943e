"""Child process of tests/test_sample_gpu.py::test_two_ranks_over_gloo: rank RANK of a world_size-2 `gloo` group on the one
GPU.  Each rank draws from the posterior of its ragged `rank::2` shard of the same data with BSC, MCA, DSC, TSC, GSC, MoG
(diagonal) and MoP, given the matching rows of U (and E): its draws equal the corresponding rows of a call on the whole array,
bit for bit (sample_posterior has no collective, and a row's draws depend on that row, the parameters and its u / eps alone).
Prints "ok <rank>" on success."""
import datetime
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch
import torch.distributed as dist

from reconstruct_world2_gpu_worker import make, problems


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    from prosper_amd.utils import parallel
    D, H, Y, probs = problems()
    Y = Y[:301]
    M = 3
    rng = np.random.RandomState(32)
    U, E = rng.uniform(size=(len(Y), M)), rng.normal(size=(len(Y), M, 3))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=300))
    comm = parallel.Comm()
    failed = None
    for kind, p in probs:
        m = make(kind, D, H, comm)
        kw = {"normals": E} if kind == "gsc" else {}
        kw_mine = {"normals": E[rank::world]} if kind == "gsc" else {}
        mine, s_mine = m.sample_posterior(p, {"y": Y[rank::world]}, n_samples=M, uniforms=U[rank::world], latents=True, **kw_mine)
        whole, s_whole = m.sample_posterior(p, {"y": Y}, n_samples=M, uniforms=U, latents=True, **kw)
        assert mine.shape == (M, len(Y[rank::world]), D) and np.isfinite(mine).all(), kind
        same = np.array_equal(mine, whole[:, rank::world]) and np.array_equal(s_mine, s_whole[:, rank::world])
        bad = None if same else (kind, np.abs(mine - whole[:, rank::world]).max())
        print("rank %d %s draws %s" % (rank, kind, "equal" if bad is None else "DIFFER %r" % (bad,)))
        failed = failed or bad
    assert not failed, failed
    dist.barrier()
    dist.destroy_process_group()
    print("ok %d" % rank)


if __name__ == "__main__":
    main()
