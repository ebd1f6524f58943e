"""Child process of tests/test_mixture_gpu.py::test_two_ranks_over_gloo: rank RANK of a world_size-2 `gloo` group; both
ranks drive the one GPU, each on its `stride_data` shard of the golden data.  Three EM steps of MoG (diagonal and full) and
MoP (A = 10 D): after every step the two ranks hold bitwise identical parameters (one packed all-reduce of statistics
summed in a fixed order, then the same host arithmetic), and the first step matches the reference's single-process step.
Prints "ok <rank>" on success."""
import datetime
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch
import torch.distributed as dist


class An(dict):
    def __missing__(self, k):
        return 0.0


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=300))
    from conftest import golden
    from prosper_amd.utils import parallel
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.em.mixturemodels.MoP import MoP
    comm = parallel.Comm()
    for case in ("mog_diag_big", "mog_full_T1", "mop_A"):
        g = golden("mixture_step_%s.npz" % case)
        D, H = int(g["D"]), int(g["H"])
        if "sigmas_sq_type" in g:
            m = MoG(D, H, sigmas_sq_type=str(g["sigmas_sq_type"]), comm=comm)
        else:
            m = MoP(D, H, A=float(g["A"]), comm=comm)
        y = g["y"][rank::world]           # ragged shards
        p = {k[3:]: np.array(v) for k, v in g.items() if k.startswith("in_")}
        for step in range(3):
            ss = m.E_step(An(T=float(g["T"])), p, {"y": y})
            p = m.M_step(An(T=float(g["T"])), {k: v.copy() for k, v in p.items()}, ss, {"y": y})
            mine = np.concatenate([np.ravel(p[k]) for k in sorted(p)])
            both = comm.allgather(mine)
            assert np.array_equal(both[0], both[1]), (case, step)
            if step == 0:
                for k in p:
                    ref = g["out_" + k]
                    np.testing.assert_allclose(p[k], ref, rtol=1e-9, atol=1e-12 * max(1.0, np.abs(ref).max()),
                                               err_msg="%s %s" % (case, k))
    dist.barrier()
    dist.destroy_process_group()
    print("ok %d" % rank)


if __name__ == "__main__":
    main()
