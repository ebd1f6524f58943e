"""Child process of tests/test_loglik_gpu.py::test_two_ranks_over_gloo: rank RANK of a world_size-2 `gloo` group on the one
GPU.  Each rank scores its ragged `rank::2` shard of the same held-out data with BSC, GSC and MoG (diagonal): the collective
total is the same bits on both ranks and equals the single-process total within 1e-12.  Prints "ok <rank>" on success."""
import datetime
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.distributed as dist


def problems():
    rng = np.random.RandomState(21)
    D, H, N = 32, 16, 1001
    bsc = {"W": rng.normal(size=(D, H)), "pi": 2.0 / H, "sigma": 1.1}
    Q = rng.normal(size=(H, H)) * 0.1
    gsc = {"W": rng.normal(size=(D, H)), "pi": np.full(H, 2.0 / H), "mu": rng.normal(size=H),
           "psi_sq": np.eye(H) + Q @ Q.T, "sigma_sq": np.float64(0.8)}
    mog = {"W": rng.normal(size=(D, H)), "pies": np.full(H, 1.0 / H), "sigmas_sq": rng.uniform(0.5, 2.0, size=(H, D))}
    Y = rng.normal(size=(N, D)) * 1.3
    return D, H, Y, [("bsc", bsc), ("gsc", gsc), ("mog", mog)]


def make(kind, D, H, comm):
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.gsc_et import GSC
    from prosper_amd.em.mixturemodels.MoG import MoG
    if kind == "bsc":
        return BSC_ET(D, H, 6, 3, comm=comm)
    if kind == "gsc":
        return GSC(D, H, 5, 3, comm=comm)
    return MoG(D, H, sigmas_sq_type="diagonal", comm=comm)


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    from prosper_amd.utils import parallel
    D, H, Y, probs = problems()
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=300))
    comm = parallel.Comm()
    for kind, p in probs:
        m = make(kind, D, H, comm)
        tot = m.log_likelihood(p, {"y": Y[rank::world]})
        both = comm.allgather(tot)
        assert both[0] == both[1], (kind, both)
        rows = np.concatenate(comm.allgather(m.log_likelihood(p, {"y": Y[rank::world]}, per_datapoint=True)))
        assert np.isfinite(tot) and abs(tot - rows.sum()) <= 1e-12 * abs(tot), (kind, tot, rows.sum())
        ref = float(os.environ["LL_REF_" + kind.upper()])
        assert abs(tot - ref) <= 1e-12 * abs(ref), (kind, tot, ref)
    dist.barrier()
    dist.destroy_process_group()
    print("ok %d" % rank)


if __name__ == "__main__":
    main()
