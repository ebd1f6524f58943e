"""Mixture models on the MI355X: ms per E-step and per EM iteration (device events after warm-up), datapoints/s and the
fraction of the f64 MFMA roof (78.6 TF/s) for flops computed from the shapes.  One JSON line per model.

    python scratch/bench_mixture.py [--iters 5] [--N 200000]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROOF = 78.6e12


class An(dict):
    def __missing__(self, k):
        return 0.0


def flops(kind, N, D, H):
    """Algorithmic f64 flops of one E-step and one M-step (multiply-add = 2)."""
    if kind == "mog_diag":
        return 2 * N * (2 * D) * H, 2 * N * (2 * D) * H
    if kind == "mop":
        return 2 * N * D * H, 2 * N * D * H
    return 2 * N * D * D * H, 2 * N * D * D * H + 2 * N * D * H      # full: maha GEMMs; Gram matrices + Y^T P


def run(kind, N, D, H, iters):
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.em.mixturemodels.MoP import MoP
    rng = np.random.RandomState(0)
    W = rng.uniform(1.0, 3.0, size=(D, H))
    y = W.T[rng.randint(H, size=N)] + 0.5 * rng.normal(size=(N, D))
    pies = np.ones(H) / H
    if kind == "mop":
        y = np.floor(np.abs(y) * 2)
        m, p = MoP(D, H), {"W": W, "pies": pies}
    elif kind == "mog_diag":
        m, p = MoG(D, H, sigmas_sq_type="diagonal"), {"W": W, "pies": pies, "sigmas_sq": np.ones((H, D))}
    else:
        m, p = MoG(D, H, sigmas_sq_type="full"), {"W": W, "pies": pies, "sigmas_sq": np.array([np.eye(D)] * H)}
    data = {"y": y}
    a = An(T=1.0)
    for _ in range(2):                                    # warm-up (upload, workspaces, code objects)
        m.M_step(a, dict(p), m.E_step(a, dict(p), data), data)
    torch.cuda.synchronize()
    e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
    t_e, t_it = [], []
    for _ in range(iters):
        e0.record()
        ss = m.E_step(a, dict(p), data)
        e1.record()
        m.M_step(a, dict(p), ss, data)
        e2.record()
        torch.cuda.synchronize()
        t_e.append(e0.elapsed_time(e1))
        t_it.append(e0.elapsed_time(e2))
    fe, fm = flops(kind, N, D, H)
    ms_e, ms_it = float(np.median(t_e)), float(np.median(t_it))
    return {"model": kind, "N": N, "D": D, "H": H, "ms_estep": round(ms_e, 3), "ms_em_iter": round(ms_it, 3),
            "datapoints_per_s": round(N / (ms_it * 1e-3)), "flop_em_iter": fe + fm,
            "roof_ms": round((fe + fm) / ROOF * 1e3, 3), "roof_fraction_estep": round(fe / ROOF / (ms_e * 1e-3), 3),
            "roof_fraction_em_iter": round((fe + fm) / ROOF / (ms_it * 1e-3), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--N", type=int, default=200000)
    ap.add_argument("--models", default="mog_diag,mop,mog_full")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    shapes = {"mog_diag": (1024, 256), "mop": (1024, 256), "mog_full": (128, 64)}
    for kind in args.models.split(","):
        D, H = shapes[kind]
        print(json.dumps(run(kind, args.N, D, H, args.iters)), flush=True)


if __name__ == "__main__":
    main()
