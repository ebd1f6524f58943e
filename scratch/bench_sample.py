"""sample_posterior(device=True, n_samples=8) next to reconstruct(device=True) of the same shape, in one process:
BSC at config 2 (D = 1024, H = 256, H' = 8, gamma = 4, N = 200 000) and MCA at config 5 (D = 256, H = 128, H' = 8, gamma = 3,
N = 100 000).  Median of synchronised calls after warm-up, the two interleaved; per-label device times of one more call
(KernelTimer).  Prints one JSON line per configuration.
usage: python scratch/bench_sample.py [--config bsc|mca|both] [--samples 8] [--repeats 9] [--warmup 2] [--scale 1.0]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

CONFIGS = {"bsc": dict(D=1024, H=256, Hprime=8, gamma=4, N=200000), "mca": dict(D=256, H=128, Hprime=8, gamma=3, N=100000)}


def problem(kind, c, dev, scale):
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    g = torch.Generator(device=dev).manual_seed(0)
    N, D, H = max(1, int(c["N"] * scale)), c["D"], c["H"]
    pi = 2.0 / H
    S = (torch.rand((N, H), generator=g, device=dev) < pi).to(torch.float64)
    if kind == "bsc":
        W = torch.randn((D, H), generator=g, device=dev, dtype=torch.float64)
        Y = S @ W.t() + torch.randn((N, D), generator=g, device=dev, dtype=torch.float64)
        model = BSC_ET(D, H, c["Hprime"], c["gamma"])
    else:
        W = 0.2 + 2.8 * torch.rand((D, H), generator=g, device=dev, dtype=torch.float64)
        Y = torch.cat([(S[i:i + 1024, None, :] * W[None, :, :]).amax(dim=2) for i in range(0, N, 1024)])     # max over the causes
        Y = Y + 0.5 * torch.randn((N, D), generator=g, device=dev, dtype=torch.float64)
        model = MCA_ET(D, H, c["Hprime"], c["gamma"])
    params = {"W": W.cpu().numpy(), "pi": pi, "sigma": 1.0 if kind == "bsc" else 0.5}
    return model, params, Y, N


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="both", choices=["bsc", "mca", "both"])
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the configuration's N (a quick look)")
    a = ap.parse_args()
    from prosper_amd.em.camodels._device import KernelTimer
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    for kind in (["bsc", "mca"] if a.config == "both" else [a.config]):
        c = CONFIGS[kind]
        model, params, Y, N = problem(kind, c, dev, a.scale)
        data = {"y": Y}

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            del out
            return (time.perf_counter() - t0) * 1e3
        ts, tr = [], []
        for i in range(a.warmup + a.repeats):
            ds = timed(lambda: model.sample_posterior(params, data, n_samples=a.samples, seed=i, device=True))
            dr = timed(lambda: model.reconstruct(params, data, device=True))
            if i >= a.warmup:
                ts.append(ds)
                tr.append(dr)
        model.timer = KernelTimer()
        timed(lambda: model.sample_posterior(params, data, n_samples=a.samples, seed=0, device=True))
        labels = {k: (n, round(ms, 4)) for k, (n, ms) in model.timer.summary().items()}
        model.timer = None
        out_bytes = N * a.samples * c["D"] * 8
        print(json.dumps({"config": kind, "shape": dict(c, N=N), "n_samples": a.samples,
                          "sample_posterior_ms": float(np.median(ts)), "sample_posterior_all_ms": [round(v, 3) for v in ts],
                          "reconstruct_ms": float(np.median(tr)), "reconstruct_all_ms": [round(v, 3) for v in tr],
                          "labels_launches_avg_ms": labels, "result_bytes": out_bytes,
                          "stream_floor_ms_at_5.5TBs": out_bytes / 5.5e12 * 1e3,
                          "gathered_rows_of_W": N * a.samples * c["gamma"], "repeats": a.repeats, "warmup": a.warmup,
                          "note": "wall time of synchronised calls with device=True; device " + torch.cuda.get_device_name(0)}))
        del model, Y, data


if __name__ == "__main__":
    main()
