#!/usr/bin/env python3
"""Cost of reconstruct(exact=True) beside log_likelihood(exact=True) at the same shape, in the
same process: the bars (D = 25, H = 10) for the six component-analysis models, BSC at H = 20 and GSC at H = 14; N = 1000
rows of y ~ N(0, 4 I), data resident, a warm-up call of each, then REPS calls.  One case per process, so that a profile's
per-kernel statistics belong to one shape:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o CASE -- python scratch/recon_exact_cost.py CASE
Without a profiler it prints the wall times."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS = 3
CASES = ("bsc", "mca", "mmca", "dsc", "tsc", "gsc", "bsc20", "gsc14")


def bars_W(size, height=10.0):
    W = np.zeros((size, size, 2 * size))
    for i in range(size):
        W[i, :, i] = height
        W[:, i, size + i] = height
    return W.reshape(size * size, 2 * size)


def problem(case):
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    from prosper_amd.em.camodels.mmca_et import MMCA_ET
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    from prosper_amd.em.camodels.tsc_et import TSC_ET
    from prosper_amd.em.camodels.gsc_et import GSC
    rng = np.random.RandomState(0)
    D, H = 25, {"bsc20": 20, "gsc14": 14}.get(case, 10)
    W = bars_W(5) if H == 10 else rng.normal(size=(D, H)) * 3
    pi = 2.0 / H
    if case.startswith("bsc"):
        return BSC_ET(D, H, 5, 3), {"W": W, "pi": pi, "sigma": 2.0}
    if case in ("mca", "mmca"):
        return (MCA_ET if case == "mca" else MMCA_ET)(D, H, 5, 3), {"W": np.maximum(W, 0.05), "pi": pi, "sigma": 2.0}
    if case == "dsc":
        return DSC_ET(D, H, 5, 3, states=np.array([0., 1., 2.])), {"W": W, "pi": np.array([0.8, 0.1, 0.1]), "sigma": 2.0}
    if case == "tsc":
        return TSC_ET(D, H, 5, 3), {"W": W, "pi": pi, "sigma": 2.0}
    return GSC(D, H, 5, 3, 'scalar'), {"W": W, "pi": np.full(H, pi), "mu": np.ones(H), "psi_sq": np.eye(H),
                                       "sigma_sq": np.float64(4.0)}


def main():
    case = sys.argv[1]
    assert case in CASES, CASES
    torch.cuda.set_device(0)
    m, p = problem(case)
    data = {"y": torch.from_numpy(np.random.RandomState(1).normal(size=(1000, 25)) * 2.0).to("cuda:0")}
    out = {}
    for name, fn in (("log_likelihood", lambda: m.log_likelihood(p, data, exact=True)),
                     ("reconstruct", lambda: m.reconstruct(p, data, device=True, exact=True))):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(REPS):
            fn()
        torch.cuda.synchronize()
        out[name] = (time.perf_counter() - t0) / REPS * 1e3
    print("%s: log_likelihood(exact) %.3f ms, reconstruct(exact) %.3f ms per call (wall, data resident, %d calls)"
          % (case, out["log_likelihood"], out["reconstruct"], REPS))


if __name__ == "__main__":
    main()
