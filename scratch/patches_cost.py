#!/usr/bin/env python3
"""Cost of reconstruct_image(): BSC (D = 64, H = 128, H' = 6, gamma = 3) on a 2048 x 2048 image, 8 x 8 patches at
stride 1 (4.17 M patches), default chunk, image resident, device=True.  A warm-up call, then the mean wall time of REPS
calls.  Run it under `rocprofv3 --kernel-trace --stats -- python scratch/patches_cost.py` for the per-kernel times; without
a profiler it prints the wall time."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REPS = 3


def main():
    torch.cuda.set_device(0)
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.utils import patches as U
    rng = np.random.RandomState(0)
    size, p, D, H = 2048, 8, 64, 128
    W = rng.normal(size=(D, H))
    params = {"W": W, "pi": 2.0 / H, "sigma": 1.0}
    img = torch.from_numpy(rng.normal(size=(size, size)) * 2).to("cuda:0")
    m = BSC_ET(D, H, 6, 3)
    n_patches = (size - p + 1) ** 2
    chunk = U.CHUNK_BYTES // (16 * D) // (size - p + 1) * (size - p + 1)
    fn = lambda: m.reconstruct_image(params, img, stride=1, device=True)
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
        fn()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / REPS * 1e3
    print("reconstruct_image BSC D=%d H=%d on %d x %d, %d patches in chunks of %d: %.1f ms per call (wall, %d calls after a "
          "warm-up; %d launches of each patch kernel in all)" % (D, H, size, size, n_patches, chunk, ms, REPS,
                                                                 (REPS + 1) * -(-n_patches // chunk)), flush=True)


if __name__ == "__main__":
    main()
