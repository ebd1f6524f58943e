#!/usr/bin/env python3
"""Cost of encode() beside reconstruct() in the same process, data resident, results left on the device: BSC
config 2's shape (D = 1024, H = 256, H' = 8, gamma = 4, N = 200 000) or, with ``mca``, MCA config 5's shape (D = 256, H = 128,
H' = 8, gamma = 3, N = 100 000: one GPU's share of 800k).  The two calls interleaved, the median of REPS synchronised repeats
after a warm-up of each.  Without further arguments it prints the wall times; with ``profile`` it runs one warm-up and three
calls of each for a kernel trace of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o encode -- python scratch/encode_cost.py profile [mca]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS = 9


def main():
    from prosper_amd.em.camodels._device import DeviceArray
    profile = "profile" in sys.argv[1:]
    mca = "mca" in sys.argv[1:]
    torch.cuda.set_device(0)
    D, H, Hp, g, N = (256, 128, 8, 3, 100000) if mca else (1024, 256, 8, 4, 200000)
    rng = np.random.RandomState(0)
    W = rng.uniform(0.1, 3.0, size=(D, H)) if mca else rng.normal(size=(D, H))
    p = {"W": W, "pi": 2.0 / H, "sigma": 1.0}
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    S = (torch.rand((N, H), generator=gen, device="cuda:0", dtype=torch.float64) < 2.0 / H).to(torch.float64)
    Wt = torch.from_numpy(W.T).to("cuda:0")
    if mca:      # max-superposition of the active causes
        Y = torch.zeros((N, D), device="cuda:0", dtype=torch.float64)
        for n0 in range(0, N, 10000):
            Y[n0:n0 + 10000] = (S[n0:n0 + 10000, :, None] * Wt[None, :, :]).amax(dim=1)
    else:
        Y = S @ Wt
    Y += torch.randn((N, D), generator=gen, device="cuda:0", dtype=torch.float64)
    del S
    if mca:
        from prosper_amd.em.camodels.mca_et import MCA_ET
        m = MCA_ET(D, H, Hp, g)
    else:
        from prosper_amd.em.camodels.bsc_et import BSC_ET
        m = BSC_ET(D, H, Hp, g)
    data = {"y": DeviceArray(Y)}
    calls = {"reconstruct": lambda: m.reconstruct(p, data, device=True), "encode": lambda: m.encode(p, data, device=True)}
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
    print(("MCA config 5" if mca else "BSC config 2") + " (D=%d H=%d H'=%d gamma=%d N=%d), median of %d: reconstruct(device=True) "
          "%.2f ms, encode(device=True) %.2f ms, difference %.2f ms"
          % (D, H, Hp, g, N, len(times["encode"]), med["reconstruct"], med["encode"], med["encode"] - med["reconstruct"]))
    print("  all repeats (ms): reconstruct %s | encode %s" % (" ".join("%.2f" % t for t in times["reconstruct"]),
                                                             " ".join("%.2f" % t for t in times["encode"])))


if __name__ == "__main__":
    main()
