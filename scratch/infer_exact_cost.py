#!/usr/bin/env python3
"""Cost of inference(exact=True, topK=10) beside log_likelihood(exact=True) on the same data, in
the same process: BSC and MCA at D = 25, N = 2000 rows of y ~ N(0, 4 I), H = 10 (the bars), 16 and 20; data resident, the
calls interleaved, one warm-up of each, then the median of REPS synchronised calls (wall times of a whole call: inference
includes its marginals -- encode(exact=True)'s two sweeps, timed beside it as a call of its own -- and the download of the
dict).
    python scratch/infer_exact_cost.py [bsc|mca] [H ...]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from recon_exact_cost import bars_W      # noqa: E402

N, D = 2000, 25


def problem(name, H):
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    rng = np.random.RandomState(0)
    W = bars_W(5) if H == 10 else rng.normal(size=(D, H)) * 3
    if name == "bsc":
        return BSC_ET(D, H, 5, 3), {"W": W, "pi": 2.0 / H, "sigma": 2.0}
    return MCA_ET(D, H, 5, 3), {"W": np.maximum(W, 0.05), "pi": 2.0 / H, "sigma": 2.0}


def main():
    names = [a for a in sys.argv[1:] if a in ("bsc", "mca")] or ["bsc", "mca"]
    Hs = [int(a) for a in sys.argv[1:] if a.isdigit()] or [10, 16, 20]
    torch.cuda.set_device(0)
    data = {"y": torch.from_numpy(np.random.RandomState(1).normal(size=(N, D)) * 2.0).to("cuda:0")}
    T1 = {"T": 1.0}
    for name in names:
        for H in Hs:
            reps = 9 if H < 20 else 3
            m, p = problem(name, H)
            fns = {"log_likelihood": lambda: m.log_likelihood(p, data, exact=True),
                   "encode": lambda: m.encode(p, data, device=True, exact=True),
                   "inference": lambda: m.inference(T1, p, data, topK=10, exact=True)}
            times = {k: [] for k in fns}
            for k, fn in fns.items():
                fn()
            torch.cuda.synchronize()
            for _ in range(reps):
                for k, fn in fns.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    times[k].append((time.perf_counter() - t0) * 1e3)
            med = {k: float(np.median(v)) for k, v in times.items()}
            print("%s H=%d (D=%d N=%d), median of %d: log_likelihood(exact=True) %.2f ms, encode(exact=True, device=True) %.2f ms, "
                  "inference(exact=True, topK=10) %.2f ms, inference / log_likelihood %.2f"
                  % (name.upper(), H, D, N, reps, med["log_likelihood"], med["encode"], med["inference"],
                     med["inference"] / med["log_likelihood"]), flush=True)
            print("  all repeats (ms): " + " | ".join("%s %s" % (k, " ".join("%.2f" % t for t in times[k])) for k in fns),
                  flush=True)


if __name__ == "__main__":
    main()
