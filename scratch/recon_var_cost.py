#!/usr/bin/env python3
"""Cost of reconstruct(variance=True) beside reconstruct() at BSC config 2 (D = 1024, H = 256, H' = 8, gamma = 4,
N = 200 000, data resident, results left on the device): the two calls interleaved, the median of REPS synchronised repeats
after a warm-up of each.  Without arguments it prints the wall times; with ``profile`` it runs one warm-up and three calls of
each for a profile of its own; with ``mca`` the shape is MCA at D = 1024 (H = 64, H' = 6, gamma = 3, N = 20 000):
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o recon_var -- python scratch/recon_var_cost.py profile [mca]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS = 7


def main():
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels._device import DeviceArray
    profile = "profile" in sys.argv[1:]
    mca = "mca" in sys.argv[1:]      # MCA at D = 1024: recon_mca_var_kernel<16> (D = 1024, H = 64, H' = 6, gamma = 3, N = 20 000)
    torch.cuda.set_device(0)
    D, H, Hp, g, N = (1024, 64, 6, 3, 20000) if mca else (1024, 256, 8, 4, 200000)
    rng = np.random.RandomState(0)
    W = rng.uniform(0.1, 3.0, size=(D, H)) if mca else rng.normal(size=(D, H))
    p = {"W": W, "pi": 2.0 / H, "sigma": 1.0}
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    S = (torch.rand((N, H), generator=gen, device="cuda:0", dtype=torch.float64) < 2.0 / H).to(torch.float64)
    Y = S @ torch.from_numpy(W.T).to("cuda:0") + torch.randn((N, D), generator=gen, device="cuda:0", dtype=torch.float64)
    del S
    if mca:
        from prosper_amd.em.camodels.mca_et import MCA_ET
        m = MCA_ET(D, H, Hp, g)
    else:
        m = BSC_ET(D, H, Hp, g)
    data = {"y": DeviceArray(Y)}
    calls = {"reconstruct": lambda: m.reconstruct(p, data, device=True),
             "variance": lambda: m.reconstruct(p, data, device=True, variance=True)}
    times = {k: [] for k in calls}
    for k, fn in calls.items():       # warm-up
        fn()
    torch.cuda.synchronize()
    for _ in range(3 if profile else REPS):
        for k, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
            del out
    med = {k: float(np.median(v)) for k, v in times.items()}
    print(("MCA" if mca else "BSC config 2") + " (D=%d H=%d H'=%d gamma=%d N=%d), median of %d: reconstruct(device=True) %.2f ms, "
          "reconstruct(variance=True, device=True) %.2f ms, difference %.2f ms"
          % (D, H, Hp, g, N, len(times["variance"]), med["reconstruct"], med["variance"], med["variance"] - med["reconstruct"]))
    print("  all repeats (ms): reconstruct %s | variance %s" % (" ".join("%.2f" % t for t in times["reconstruct"]),
                                                               " ".join("%.2f" % t for t in times["variance"])))


if __name__ == "__main__":
    main()
