#!/usr/bin/env python3
"""Cost of reconstruct() beside log_likelihood() of the same call shape: BSC config 2, MCA config 5, GSC config 4,
MoG diagonal (D = 1024, H = 256).  Data resident, a warm-up call, then the mean wall time of REPS calls with device=True
(no download).  Run it under `rocprofv3 --kernel-trace --stats -- python scratch/recon_cost.py [model]` for the per-kernel
times; without a profiler it prints the wall times."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS = 5


def problems(which):
    rng = np.random.RandomState(0)
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    from prosper_amd.em.camodels.gsc_et import GSC
    from prosper_amd.em.mixturemodels.MoG import MoG
    if which == "bsc":
        D, H, N = 1024, 256, 200000
        W = rng.normal(size=(D, H))
        S = (rng.uniform(size=(N, H)) < 2.0 / H).astype(np.float64)
        return BSC_ET(D, H, 8, 4), {"W": W, "pi": 2.0 / H, "sigma": 1.0}, S @ W.T + rng.normal(size=(N, D))
    if which == "mca":
        D, H, N = 256, 128, 100000
        W = rng.uniform(0.5, 8.0, size=(D, H))
        return MCA_ET(D, H, 8, 3), {"W": W, "pi": 2.0 / H, "sigma": 1.0}, np.abs(rng.normal(size=(N, D))) * 4
    if which == "gsc":
        D, H, N = 256, 128, 200000
        W = rng.normal(size=(D, H))
        p = {"W": W, "pi": np.full(H, 2.0 / H), "mu": np.ones(H), "psi_sq": np.eye(H), "sigma_sq": np.float64(1.0)}
        S = (rng.uniform(size=(N, H)) < 2.0 / H) * (1 + rng.normal(size=(N, H)))
        return GSC(D, H, 6, 3, 'scalar'), p, S @ W.T + rng.normal(size=(N, D))
    D, H, N = 1024, 256, 200000
    W = rng.normal(size=(D, H)) * 2
    p = {"W": W, "pies": np.full(H, 1.0 / H), "sigmas_sq": np.ones((H, D))}
    return MoG(D, H, sigmas_sq_type='diagonal'), p, W.T[rng.randint(H, size=N)] + rng.normal(size=(N, D))


def main():
    torch.cuda.set_device(0)
    for which in (sys.argv[1:] or ["bsc", "mca", "gsc", "mog"]):
        m, p, Y = problems(which)
        data = {"y": torch.from_numpy(Y).to("cuda:0")}
        del Y
        out = {}
        for name, fn in (("log_likelihood", lambda: m.log_likelihood(p, data)),
                         ("reconstruct", lambda: m.reconstruct(p, data, device=True))):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(REPS):
                fn()
            torch.cuda.synchronize()
            out[name] = (time.perf_counter() - t0) / REPS * 1e3
        print("%s: log_likelihood %.2f ms, reconstruct %.2f ms per call (wall, data resident, %d calls)"
              % (which, out["log_likelihood"], out["reconstruct"], REPS), flush=True)
        del m, data
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
