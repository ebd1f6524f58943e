#!/usr/bin/env python3
"""Cost of k-means++ seeding at the mixture bench shape: N = 200 000, D = 1024, H = 256, data resident.

    python scratch/bench_seeding.py [--N 200000] [--D 1024] [--H 256] [--reps 5] [--no-numpy]

Prints the median wall time of synchronised ``kmeanspp`` calls after a warm-up beside two references measured in the same
process: H plain streaming reads of Y (``torch.sum`` over the shard) and the NumPy restatement (tests/seeding_reference.py)
at N / 10, scaled by 10.  Per-kernel times come from a rocprofv3 --kernel-trace --stats run of this script (--reps 1
--no-numpy)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from prosper_amd.utils.seeding import kmeanspp   # noqa: E402


def median_ms(fn, reps):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=200000)
    ap.add_argument("--D", type=int, default=1024)
    ap.add_argument("--H", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    Y = torch.randn((a.N, a.D), generator=g, device=dev, dtype=torch.float64)
    u = np.random.RandomState(0).uniform(size=a.H)
    gb = a.N * a.D * 8 / 1e9

    kmeanspp(Y, a.H, uniforms=u, device=True)            # warm-up
    seed_ms, seed_all = median_ms(lambda: kmeanspp(Y, a.H, uniforms=u, device=True), a.reps)

    def reads():
        for _ in range(a.H):
            torch.sum(Y)
    reads()
    read_ms, read_all = median_ms(reads, a.reps)
    rate = a.H * gb / (read_ms / 1e3) / 1e3                # TB/s of the plain reads
    print("shape N=%d D=%d H=%d: shard %.3f GB" % (a.N, a.D, a.H, gb))
    print("kmeanspp (device, resident):      %9.2f ms median of %d  %s" % (seed_ms, a.reps, ["%.1f" % t for t in seed_all]))
    print("H plain reads of Y (torch.sum):   %9.2f ms median of %d  -> %.2f TB/s" % (read_ms, a.reps, rate))
    print("kmeanspp / plain reads:           %9.2f   (%.2f TB/s of Y over the whole call)" % (
        seed_ms / read_ms, a.H * gb / (seed_ms / 1e3) / 1e3))
    print("floor H N D 8 bytes at the measured plain-read rate: %.2f ms" % read_ms)
    if not a.no_numpy:
        import seeding_reference as SR
        n = a.N // 10
        Yh = Y[:n].cpu().numpy()
        hs = 4                                               # rounds timed; a round's cost does not depend on h
        t0 = time.perf_counter()
        SR.kmeanspp([Yh], hs, u[:hs])
        per_round = (time.perf_counter() - t0) / hs
        print("NumPy restatement at N/10 = %d: %.1f ms per round -> x10 x H = %.1f s for the full shape" % (
            n, per_round * 1e3, per_round * 10 * a.H))
        t0 = time.perf_counter()
        c = Yh[0]
        for _ in range(hs):
            ((Yh - c) ** 2).sum(1)
        per_round = (time.perf_counter() - t0) / hs
        print("vectorised NumPy distance pass alone at N/10: %.1f ms per round -> x10 x H = %.1f s" % (
            per_round * 1e3, per_round * 10 * a.H))


if __name__ == "__main__":
    main()
