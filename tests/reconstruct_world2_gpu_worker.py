"""Child process of tests/test_reconstruct_gpu.py::test_two_ranks_over_gloo: rank RANK of a world_size-2 `gloo` group on the
one GPU.  Each rank reconstructs its ragged `rank::2` shard of the same data with BSC, MCA, DSC, TSC, GSC, MoG (diagonal) and
MoP: its rows equal the corresponding rows of a call on the whole array, bit for bit (reconstruct has no collective, and a
row's value does not depend on the other rows).  Prints "ok <rank>" on success."""
import datetime
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch
import torch.distributed as dist


def problems():
    rng = np.random.RandomState(31)
    D, H, N = 32, 16, 1001
    bsc = {"W": rng.normal(size=(D, H)), "pi": 2.0 / H, "sigma": 1.1, "mu": rng.normal(size=D)}
    mca = {"W": rng.uniform(0.2, 3.0, size=(D, H)), "pi": 2.0 / H, "sigma": 0.9}
    Q = rng.normal(size=(H, H)) * 0.1
    gsc = {"W": rng.normal(size=(D, H)), "pi": np.full(H, 2.0 / H), "mu": rng.normal(size=H),
           "psi_sq": np.eye(H) + Q @ Q.T, "sigma_sq": np.float64(0.8)}
    mog = {"W": rng.normal(size=(D, H)), "pies": np.full(H, 1.0 / H), "sigmas_sq": rng.uniform(0.5, 2.0, size=(H, D))}
    dsc = {"W": rng.normal(size=(D, H)), "pi": np.array([0.85, 0.1, 0.05]), "sigma": 1.0}
    tsc = {"W": rng.normal(size=(D, H)), "pi": 0.15, "sigma": 1.0}
    mop = {"W": rng.uniform(0.5, 4.0, size=(D, H)), "pies": np.full(H, 1.0 / H)}
    Y = np.round(np.abs(rng.normal(size=(N, D))) * 1.3 * 2) / 2
    return D, H, Y, [("bsc", bsc), ("mca", mca), ("dsc", dsc), ("tsc", tsc), ("gsc", gsc), ("mog", mog), ("mop", mop)]


def make(kind, D, H, comm):
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    from prosper_amd.em.camodels.gsc_et import GSC
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    from prosper_amd.em.camodels.tsc_et import TSC_ET
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.em.mixturemodels.MoP import MoP
    if kind == "dsc":
        return DSC_ET(D, H, 5, 3, states=np.array([0., 1., 2.]), comm=comm)
    if kind == "tsc":
        return TSC_ET(D, H, 5, 3, comm=comm)
    if kind == "mop":
        return MoP(D, H, comm=comm)
    if kind == "bsc":
        return BSC_ET(D, H, 6, 3, comm=comm)
    if kind == "mca":
        return MCA_ET(D, H, 6, 3, comm=comm)
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
    failed = None
    for kind, p in probs:
        m = make(kind, D, H, comm)
        mine = m.reconstruct(p, {"y": Y[rank::world]})
        whole = m.reconstruct(p, {"y": Y})
        assert mine.shape == (len(Y[rank::world]), D) and np.isfinite(mine).all(), kind
        bad = None if np.array_equal(mine, whole[rank::world]) else (kind, np.abs(mine - whole[rank::world]).max())
        print("rank %d %s rows %s" % (rank, kind, "equal" if bad is None else "DIFFER %r" % (bad,)))
        failed = failed or bad
    assert not failed, failed
    dist.barrier()
    dist.destroy_process_group()
    print("ok %d" % rank)


if __name__ == "__main__":
    main()
