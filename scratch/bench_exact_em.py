#!/usr/bin/env python3
"""Cost record of the exact EM step: one ``exact_step`` beside ``reconstruct(exact=True, device=True)`` on the
same rows in the same process, data resident; median of synchronised repeats after a warm-up of each.

    python scratch/bench_exact_em.py [--repeats 7] [--once]

``--once`` (for a kernel trace): one warm-up and one call of each per shape."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    reps = 1 if a.once else a.repeats

    class Anneal(dict):
        def __missing__(self, key):
            return 0.0

        def as_dict(self):
            return dict(self)

    for D, H, N in ((64, 16, 10000), (64, 20, 2000)):
        rng = np.random.RandomState(H)
        Wg = 3.0 * rng.normal(size=(D, H))
        Y = (rng.random_sample((N, H)) < 2.0 / H) @ Wg.T + rng.normal(size=(N, D))
        params = {"W": Wg + 0.1 * rng.normal(size=(D, H)), "pi": 2.0 / H, "sigma": 1.05}
        m = BSC_ET(D, H, 5, 3)
        data = {"y": torch.from_numpy(Y).cuda()}
        an = Anneal(T=1.0)
        times = {"exact_step": [], "reconstruct": []}
        for i in range(reps + 1):
            for what in ("reconstruct", "exact_step"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if what == "exact_step":
                    m.exact_step(an, dict(params), data)
                else:
                    m.reconstruct(dict(params), data, exact=True, device=True)
                torch.cuda.synchronize()
                if i:
                    times[what].append((time.perf_counter() - t0) * 1e3)
        ms = {k: float(np.median(v)) for k, v in times.items()}
        print("BSC D=%d H=%d N=%d, median of %d: reconstruct(exact=True) %.2f ms, exact_step %.2f ms, ratio %.2f "
              "(sweeps: (3 + (H - 10) / 2) / 2 = %.2f)" % (D, H, N, reps, ms["reconstruct"], ms["exact_step"],
                                                              ms["exact_step"] / ms["reconstruct"], 1.5 + (H - 10) / 4.0))
        print("  all repeats (ms): reconstruct %s | exact_step %s" % (" ".join("%.2f" % t for t in times["reconstruct"]),
                                                                     " ".join("%.2f" % t for t in times["exact_step"])))


if __name__ == "__main__":
    main()
