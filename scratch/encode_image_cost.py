"""Cost of encode_image(pool=2) on one 512 x 512 image (p = 8, stride 1: 505^2 = 255 025 patches) with BSC at D = H = 64,
split into its three parts -- patch extraction, encode(), pooling of both codes -- each timed on its own over resident
inputs, and the pooling pass's achieved read rate beside torch.sum over the same code buffer (the yardstick of
scratch/bw_probe.py).  Wall times around a device synchronise, median of nine after one warm-up, the parts interleaved.

    python scratch/encode_image_cost.py [output file]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from prosper_amd.em.camodels._device import DeviceArray        # noqa: E402
from prosper_amd.em.camodels.bsc_et import BSC_ET              # noqa: E402
from prosper_amd.utils import patches as U                     # noqa: E402

SIZE, P, H, HP, GAMMA, POOL, REPS = 512, 8, 64, 8, 3, (2, 2), 9


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    rng = np.random.RandomState(0)
    D = P * P
    model = BSC_ET(D, H, HP, GAMMA)
    params = {"W": rng.normal(size=(D, H)), "pi": 2.0 / H, "sigma": 1.0}
    image = torch.from_numpy(rng.normal(size=(SIZE, SIZE)) * 2.0).to(dev)
    geo = U._geometry((SIZE, SIZE), P, 1)
    _, _, _, nr, nc = geo
    N, grid = nr * nc, (1, nr, nc)
    img, ldi = U._image_tensor(image, dev)
    Y = U._extract(img, ldi, geo, 0, N, False, False)[0]
    mean, prob = (t.tensor for t in model.encode(params, {"y": DeviceArray(Y)}, device=True))
    work = U._pool_work(nr, nc, POOL[1], H, dev)

    def pool_both(reduce="mean"):
        for codes in (mean, prob):
            acc = U._pool_begin(grid, POOL, H, reduce, dev)
            U._pool(acc, codes, H, grid, POOL, 0, N, reduce, work, False)
            U._pool_finish(acc, grid, POOL, reduce, False)

    parts = {
        "encode_image(pool=2)": lambda: model.encode_image(params, image, pool=2, device=True),
        "extract": lambda: U._extract(img, ldi, geo, 0, N, False, False),
        "encode": lambda: model.encode(params, {"y": DeviceArray(Y)}, device=True),
        "pool (both codes)": pool_both,
        "pool max (both codes)": lambda: pool_both("max"),
        "torch.sum (both codes)": lambda: (mean.sum(), prob.sum()),
        "torch.sum(dim=0) (both codes)": lambda: (mean.sum(dim=0), prob.sum(dim=0)),
    }
    times = {k: [] for k in parts}
    for k, fn in parts.items():
        timed(fn)                                               # warm-up of every shape
    for _ in range(REPS):
        for k, fn in parts.items():
            times[k].append(timed(fn))
    med = {k: statistics.median(v) for k, v in times.items()}
    nbytes = 2 * N * H * 8
    lines = ["# scratch/encode_image_cost.py on one %s: BSC D=%d H=%d H'=%d gamma=%d, one %d x %d image, p=%d, stride 1, "
             "N=%d patches, pool=%r" % (torch.cuda.get_device_name(0), D, H, HP, GAMMA, SIZE, SIZE, P, N, POOL),
             "# wall times of whole calls around a device synchronise, inputs resident, median of %d after one warm-up, the "
             "parts interleaved in one process" % REPS]
    for k in parts:
        lines.append("%-32s median %8.3f ms   all: %s" % (k, med[k], " ".join("%.3f" % v for v in times[k])))
    whole = med["encode_image(pool=2)"]
    lines.append("shares of the whole call: extract %.1f %%, encode %.1f %%, pooling %.1f %% (parts timed on their own: they need "
                 "not add up to the whole)" % tuple(100 * med[k] / whole for k in ("extract", "encode", "pool (both codes)")))
    lines.append("pooling reads both code buffers once: %.1f MB in %.3f ms = %.2f TB/s (launch and synchronise included; six "
                 "launches)" % (nbytes / 1e6, med["pool (both codes)"], nbytes / med["pool (both codes)"] / 1e9))
    for k in ("torch.sum (both codes)", "torch.sum(dim=0) (both codes)"):
        lines.append("yardstick %s over the same buffers: %.3f ms = %.2f TB/s" % (k, med[k], nbytes / med[k] / 1e9))
    lines.append("# the code buffers (2 x %.0f MB) fit the 256 MiB Infinity Cache and were written just before: both rates are "
                 "cache-assisted, which is the situation inside encode_image as well" % (nbytes / 2e6))
    lines.append("# No kernel trace was taken: per-kernel times are not measured.")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
