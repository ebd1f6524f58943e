"""Child process of tests/test_loglik_exact_gpu.py::test_two_ranks_over_gloo: rank RANK of a world_size-2 `gloo` group on the
one GPU.  Each rank scores its ragged `rank::2` shard of the same held-out data with log_likelihood(..., exact=True) for BSC
and GSC: the collective total is the same bits on both ranks and is the rank-ordered sum of the per-rank totals (each taken
on a one-rank group).  Prints "ok <rank>" on success."""
import datetime
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.distributed as dist


def problems():
    rng = np.random.RandomState(22)
    D, H, N = 12, 10, 1001
    bsc = {"W": rng.normal(size=(D, H)), "pi": 2.0 / H, "sigma": 1.1}
    Q = rng.normal(size=(H, H)) * 0.1
    gsc = {"W": rng.normal(size=(D, H)), "pi": np.full(H, 2.0 / H), "mu": rng.normal(size=H),
           "psi_sq": np.eye(H) + Q @ Q.T, "sigma_sq": np.float64(0.8)}
    Y = rng.normal(size=(N, D)) * 1.3
    return D, H, Y, [("bsc", bsc), ("gsc", gsc)]


def make(kind, D, H, comm):
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.gsc_et import GSC
    return BSC_ET(D, H, 6, 3, comm=comm) if kind == "bsc" else GSC(D, H, 5, 3, comm=comm)


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    from prosper_amd.utils import parallel
    D, H, Y, probs = problems()
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=300))
    comm = parallel.Comm()
    solo = [dist.new_group([r]) for r in range(world)]
    one = parallel.Comm(solo[rank])
    assert one.size == 1
    for kind, p in probs:
        shard = {"y": Y[rank::world]}
        tot = make(kind, D, H, comm).log_likelihood(p, shard, exact=True)
        both = comm.allgather(tot)
        assert both[0] == both[1], (kind, both)
        local = make(kind, D, H, one).log_likelihood(p, shard, exact=True)
        want = 0.0
        for v in comm.allgather(local):
            want += v
        assert np.isfinite(tot) and tot == want, (kind, tot, want)
        rows = np.concatenate(comm.allgather(make(kind, D, H, one).log_likelihood(p, shard, per_datapoint=True,
                                                                                  exact=True)))
        assert abs(tot - rows.sum()) <= 1e-12 * abs(tot), (kind, tot, rows.sum())
    dist.barrier()
    dist.destroy_process_group()
    print("ok %d" % rank)


if __name__ == "__main__":
    main()
