"""Child process of tests/test_seeding_gpu.py::test_two_ranks_over_gloo and ::test_forced_collectives_on_one_rank_give_the_
one_rank_bits: rank RANK of a world_size-WORLD_SIZE `gloo` group on the one GPU.  Each rank seeds from its contiguous, ragged
shard of the same data: every rank holds the same centres, global indices and potentials, equal bit for bit to
tests/seeding_reference.py run on the shards with the rank-order rule (one shard: the one-rank rule), for ``kmeanspp`` and
for ``kmeanspp_init`` of MoG (diagonal) and MoP.  Prints "ok <rank>" on success."""
import datetime
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch
import torch.distributed as dist

import seeding_reference as SR


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    from prosper_amd.utils import parallel
    from prosper_amd.utils.seeding import kmeanspp
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.em.mixturemodels.MoP import MoP
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=300))
    comm = parallel.Comm()
    assert not comm._solo()
    rng = np.random.RandomState(41)
    N, D, H = 777, 33, 9
    Y = rng.normal(size=(N, D)) * 2.0
    u = rng.uniform(size=H)
    cut = [0, 400, N] if world == 2 else [0, N]           # ragged shards
    shards = [Y[cut[r]:cut[r + 1]] for r in range(world)]
    want = SR.kmeanspp(shards, H, u)[:3]
    c, i, p = kmeanspp(shards[rank], H, uniforms=u, comm=comm)
    assert np.array_equal(i, want[1]) and np.array_equal(_bits(p), _bits(want[2])) and np.array_equal(_bits(c), _bits(want[0]))
    assert np.array_equal(_bits(c), _bits(Y[i])) and len(set(i.tolist())) == H
    both = comm.allgather(np.concatenate([c.ravel(), i.astype(np.float64), p]))
    assert all(np.array_equal(_bits(b), _bits(both[0])) for b in both)
    if world == 1:
        from prosper_amd.utils.parallel import Comm
        solo = kmeanspp(Y, H, uniforms=u, comm=Comm(force_collectives=False))
        assert np.array_equal(solo[1], i) and np.array_equal(_bits(solo[2]), _bits(p)) and np.array_equal(_bits(solo[0]), _bits(c))
    # the seeded form draws on rank 0 and broadcasts
    s = kmeanspp(shards[rank], H, seed=11, comm=comm)
    both = comm.allgather(s[1])
    assert all(np.array_equal(b, both[0]) for b in both) and len(set(s[1].tolist())) == H
    # data with too few distinct rows: every rank raises after the rounds
    dup = Y[:4][rng.randint(0, 4, size=N)]
    try:
        kmeanspp(dup[cut[rank]:cut[rank + 1]], H, uniforms=u, comm=comm)
        raise AssertionError("no error for 4 distinct rows")
    except ValueError as e:
        assert "round 4" in str(e), e
    for m, data in ((MoG(D, H, sigmas_sq_type='diagonal', comm=comm), Y), (MoP(D, H, comm=comm), np.abs(Y) + 0.5)):
        sh = [data[cut[r]:cut[r + 1]] for r in range(world)]
        w = SR.kmeanspp(sh, H, u)[:3]
        q = m.kmeanspp_init({'y': sh[rank]}, uniforms=u)
        assert np.array_equal(_bits(q['W']), _bits(m._seed_rates(w[0].T))) and np.array_equal(m.seed_indices, w[1])
        both = comm.allgather(np.concatenate([np.ravel(q[k]) for k in sorted(q)]))
        assert all(np.array_equal(_bits(b), _bits(both[0])) for b in both)
    dist.barrier()
    dist.destroy_process_group()
    print("ok %d" % rank)


if __name__ == "__main__":
    main()
