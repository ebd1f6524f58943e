#!/usr/bin/env python3
"""Cost of a weighted reconstruct beside the masked reconstruct with the same zero pattern (existing
code, the yardstick): BSC config 2 (D = 1024, H = 256, H' = 8, gamma = 4, N = 200 000) and MCA config 5 (D = 256, H = 128,
H' = 8, gamma = 3, N = 100 000), 50 % zero weights, the rest uniform in [0.25, 4]; data, mask and weights resident on the
device, device=True, both calls in one process.  After WARMUP calls of each the two are timed alternately, REPS times, every
call between two device synchronisations; the medians are printed, and beside them what the weighted call reads more than the
masked one: the weight (N D 8 bytes) where the masked call reads a mask byte (N D), once in prepare and once in the row
kernel -- the two GEMM operands are N x D doubles in both calls (X0 / Mf there, Xw / Om here)."""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARMUP, REPS = 3, 9


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def run(name, model, p, Y, mask, weight):
    from prosper_amd.em.camodels._device import DeviceArray
    dm = {"y": DeviceArray(Y), "mask": DeviceArray(mask)}
    dw = {"y": DeviceArray(Y), "weight": DeviceArray(weight)}
    f_m = lambda: model.reconstruct(p, dm, device=True)
    f_w = lambda: model.reconstruct(p, dw, device=True)
    for _ in range(WARMUP):
        f_m()
        f_w()
    tm, tw = [], []
    for _ in range(REPS):
        tm.append(timed(f_m))
        tw.append(timed(f_w))
    N, D = Y.shape
    med_m, med_w = statistics.median(tm), statistics.median(tw)
    extra = N * D * 8 / 1e9
    print("%s, median of %d: masked reconstruct %.2f ms, weighted reconstruct %.2f ms, difference %+.2f ms" % (
        name, REPS, med_m, med_w, med_w - med_m))
    print("  the weight is N D 8 = %.2f GB against N D = %.2f GB of mask bytes: read once in prepare and once in the row kernel "
          "(%.2f GB more, %.2f ms at 5 TB/s)" % (extra, extra / 8, 2 * extra * 7 / 8, 2 * extra * 7 / 8 / 5.0))
    print("  all repeats (ms): masked %s | weighted %s" % (" ".join("%.2f" % t for t in tm), " ".join("%.2f" % t for t in tw)))


def main():
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    rng = np.random.RandomState(0)

    def observation(N, D):
        mask = torch.rand(N, D, generator=g, device=dev) < 0.5
        weight = torch.where(mask, 0.25 + 3.75 * torch.rand(N, D, generator=g, device=dev, dtype=torch.float64),
                             torch.zeros((), dtype=torch.float64, device=dev))
        return mask.view(torch.uint8), weight

    D, H, N = 1024, 256, 200_000
    W = rng.normal(size=(D, H))
    S = (torch.rand(N, H, generator=g, device=dev) < 2.0 / H).to(torch.float64)
    Y = S @ torch.from_numpy(W.T).to(dev) + torch.randn(N, D, generator=g, device=dev, dtype=torch.float64)
    mask, weight = observation(N, D)
    run("BSC config 2 (D=1024 H=256 H'=8 gamma=4 N=200000)", BSC_ET(D, H, 8, 4), {"W": W, "pi": 2.0 / H, "sigma": 1.0}, Y, mask,
        weight)
    del Y, S, mask, weight
    torch.cuda.empty_cache()

    D, H, N = 256, 128, 100_000
    W = np.abs(rng.normal(size=(D, H))) * 2 + 0.1
    Y = torch.rand(N, D, generator=g, device=dev, dtype=torch.float64) * 3
    mask, weight = observation(N, D)
    run("MCA config 5 (D=256 H=128 H'=8 gamma=3 N=100000)", MCA_ET(D, H, 8, 3), {"W": W, "pi": 2.0 / H, "sigma": 1.0}, Y, mask,
        weight)


if __name__ == "__main__":
    main()
