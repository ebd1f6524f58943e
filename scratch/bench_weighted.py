#!/usr/bin/env python3
"""Cost of the precision-weighted aggregate against the plain overlap average: BSC (D = 64, H = 128, H' = 6,
gamma = 3) on a 512 x 512 image, 8 x 8 patches at stride 1 (255 025 patches), image resident, device=True, both aggregates in
one process.  After WARMUP calls of each the two are timed alternately, REPS times, every call between two device
synchronisations; the median wall time of each is printed, and beside it the accumulate kernels alone (the plain one and
the weighted one on the same estimate and variance rows, same protocol)."""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WARMUP, REPS = 3, 15


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def interleaved(fns):
    for fn in fns:
        for _ in range(WARMUP):
            fn()
    times = [[] for _ in fns]
    for _ in range(REPS):
        for t, fn in zip(times, fns):
            t.append(timed(fn))
    return [statistics.median(t) for t in times]


def main():
    torch.cuda.set_device(0)
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.utils import patches as U
    rng = np.random.RandomState(0)
    size, p, D, H = 512, 8, 64, 128
    params = {"W": rng.normal(size=(D, H)), "pi": 2.0 / H, "sigma": 1.0}
    img = torch.from_numpy(rng.normal(size=(size, size)) * 2).to("cuda:0")
    m = BSC_ET(D, H, 6, 3)
    N = (size - p + 1) ** 2
    mean, prec, mean_var = interleaved([lambda: m.reconstruct_image(params, img, device=True),
                                        lambda: m.reconstruct_image(params, img, device=True, aggregate='precision'),
                                        lambda: m.reconstruct_image(params, img, device=True, variance=True)])
    print("reconstruct_image BSC D=%d H=%d on %d x %d, %d patches, median of %d synchronised calls after %d warm-ups: mean "
          "aggregate %.2f ms, precision aggregate %.2f ms (mean aggregate with variance=True, which runs the same "
          "reconstruct(): %.2f ms)" % (D, H, size, size, N, REPS, WARMUP, mean, prec, mean_var), flush=True)
    # the accumulate kernels alone
    geo = U._geometry((size, size), p, 1)
    Y, _ = U._extract(img[None], size, geo, 0, N, False, False)
    V = torch.rand((N, D), dtype=torch.float64, device=img.device)
    acc, den = torch.zeros((1, size, size), dtype=torch.float64, device=img.device), torch.zeros((1, size, size), dtype=torch.float64, device=img.device)
    plain, weighted = interleaved([lambda: U._accumulate(acc, Y, D, None, geo, 0, N, False),
                                   lambda: U._accumulate_w(acc, den, Y, D, V, D, 1, 0.5, None, None, geo, 0, N, False)])
    print("accumulate alone (one launch and its synchronisation; %.0f MB of estimate rows, twice that with the variances): "
          "plain %.3f ms, weighted %.3f ms" % (N * D * 8 / 1e6, plain, weighted), flush=True)


if __name__ == "__main__":
    main()
