"""One masked BSC EM step at config 2's shape next to the unmasked step, in one process: median of synchronised
repeats after warm-up, the two interleaved.  Prints one JSON line.
usage: python scratch/bench_masked_train.py [--N 200000] [--repeats 5] [--warmup 2] [--labels]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch


class Anneal(dict):
    def __missing__(self, key):
        return 0.0

    def as_dict(self):
        return dict(self)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=200000)
    ap.add_argument("--D", type=int, default=1024)
    ap.add_argument("--H", type=int, default=256)
    ap.add_argument("--Hprime", type=int, default=8)
    ap.add_argument("--gamma", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--labels", action="store_true", help="per-label device times of one more masked step (KernelTimer)")
    a = ap.parse_args()
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels._device import KernelTimer
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    N, D, H = a.N, a.D, a.H
    pi = 2.0 / H
    W = torch.randn((D, H), generator=g, device=dev, dtype=torch.float64)
    S = (torch.rand((N, H), generator=g, device=dev) < pi).to(torch.float64)
    Y = S @ W.t() + torch.randn((N, D), generator=g, device=dev, dtype=torch.float64)
    M = (torch.rand((N, D), generator=g, device=dev) < 0.5).to(torch.uint8)
    del S
    params = {"W": (W + 0.1 * torch.randn((D, H), generator=g, device=dev, dtype=torch.float64)).cpu().numpy(),
              "pi": pi * 1.1, "sigma": 1.05}
    an = Anneal(T=1.0)
    masked, plain = BSC_ET(D, H, a.Hprime, a.gamma), BSC_ET(D, H, a.Hprime, a.gamma)
    data_m, data_p = {"y": Y, "mask": M}, {"y": Y}

    def timed(model, data):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.step(an, dict(params), data)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    tm, tp = [], []
    for i in range(a.warmup + a.repeats):
        dm, out = timed(masked, data_m)
        dp, _ = timed(plain, data_p)
        if i >= a.warmup:
            tm.append(dm)
            tp.append(dp)
    res = {"shape": {"N": N, "D": D, "H": H, "Hprime": a.Hprime, "gamma": a.gamma, "observed": 0.5},
           "masked_step_ms": float(np.median(tm)), "masked_step_all_ms": [round(v, 2) for v in tm],
           "unmasked_step_ms": float(np.median(tp)), "unmasked_step_all_ms": [round(v, 3) for v in tp],
           "W_kept": masked.W_kept, "finite": bool(np.isfinite(out["W"]).all()), "repeats": a.repeats, "warmup": a.warmup,
           "note": "wall time of one synchronised step() with the same (cold) parameters every time; device "
                   + torch.cuda.get_device_name(0)}
    if a.labels:
        masked.timer = KernelTimer()
        timed(masked, data_m)
        res["masked_labels_ms"] = masked.timer.summary()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
