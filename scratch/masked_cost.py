#!/usr/bin/env python3
"""Cost of the masked reconstruct() beside the unmasked call of the same shape, in one process: BSC config 2
(D = 1024, H = 256, N = 200 000, H' = 8, gamma = 4) and MCA config 5 (D = 256, H = 128, N = 100 000, H' = 8, gamma = 3), 50 % of
the entries observed.  Data and mask resident, device=True (no download), two warm-up calls, then the MEDIAN wall time of
REPS synchronised calls, the two variants interleaved.  Run it under
`rocprofv3 --kernel-trace --stats -- python scratch/masked_cost.py [model]` for the per-kernel times (a run of its own: the
wall times of a profiled run are not the ones to quote)."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS = 9


def problems(which):
    rng = np.random.RandomState(0)
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    if which == "bsc":
        D, H, N = 1024, 256, 200000
        W = rng.normal(size=(D, H))
        S = (rng.uniform(size=(N, H)) < 2.0 / H).astype(np.float64)
        return BSC_ET(D, H, 8, 4), {"W": W, "pi": 2.0 / H, "sigma": 1.0}, S @ W.T + rng.normal(size=(N, D))
    D, H, N = 256, 128, 100000
    W = rng.uniform(0.5, 8.0, size=(D, H))
    return MCA_ET(D, H, 8, 3), {"W": W, "pi": 2.0 / H, "sigma": 1.0}, np.abs(rng.normal(size=(N, D))) * 4


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    torch.cuda.set_device(0)
    for which in (sys.argv[1:] or ["bsc", "mca"]):
        m, p, Y = problems(which)
        N, D = Y.shape
        y = torch.from_numpy(Y).to("cuda:0")
        del Y
        mask = (torch.rand((N, D), device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(1)) < 0.5).to(torch.uint8)
        plain, masked = {"y": y}, {"y": y, "mask": mask}
        calls = {"unmasked": lambda: m.reconstruct(p, plain, device=True), "masked": lambda: m.reconstruct(p, masked, device=True)}
        for fn in calls.values():
            fn()
            fn()
        times = {k: [] for k in calls}
        for _ in range(REPS):
            for k, fn in calls.items():
                times[k].append(timed(fn))
        med = {k: float(np.median(v)) for k, v in times.items()}
        print("%s (D=%d H=%d N=%d H'=%d gamma=%d, 50 %% observed): reconstruct unmasked %.2f ms [%.2f .. %.2f], masked %.2f ms "
              "[%.2f .. %.2f], ratio %.2f (median of %d synchronised calls each, data resident, device=True)"
              % (which, D, m.H, N, m.Hprime, m.gamma, med["unmasked"], min(times["unmasked"]), max(times["unmasked"]),
                 med["masked"], min(times["masked"]), max(times["masked"]), med["masked"] / med["unmasked"], REPS), flush=True)
        del m, y, mask, plain, masked, calls
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
