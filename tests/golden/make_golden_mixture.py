#!/usr/bin/env python3 -B
"""Mint golden vectors of the mixture models (MoG, MoP) from the REFERENCE itself.

Same pattern as make_golden.py (see its header): the reference is imported through the single-rank mpi4py / tables
shims in ./_shims, fed seeded inputs, and inputs + outputs are stored as small .npz files next to this script.

    python -B tests/golden/make_golden_mixture.py

Fixtures (float64, what the reference returned):
  mixture_step_<case>.npz   E_step -> M_step of MoG (diagonal / full) or MoP (A = nan / 10 D): inputs, logpj,
                            posteriors_h, new parameters; includes the clamp cases and the indefinite full covariance
  mixture_gen_init.npz      generate_data and standard_init of the three models for fixed seeds
  mixture_traj_<model>.npz  20 EM steps on bars data (D=25, H=10, N=2000; T 2 -> 1), parameters after every step
                            (MoG full: the first 3 steps -- a covariance turns singular at step 3, and past it the run is
                            chaotic: a 1e-13 perturbation grows to O(1))
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "_shims"))
sys.path.insert(1, "/root/reference")

import numpy as np

for _n, _t in (("int", int), ("bool", bool), ("str", str), ("object", object), ("float", float)):
    if _n not in np.__dict__:
        setattr(np, _n, _t)

from prosper.em.annealing import LinearAnnealing             # noqa: E402
from prosper.em.mixturemodels.MoG import MoG                 # noqa: E402
from prosper.em.mixturemodels.MoP import MoP                 # noqa: E402
from prosper.utils.barstest import generate_bars_dict        # noqa: E402
from prosper.utils.datalog import dlog                       # noqa: E402


def _anneal(T):
    a = LinearAnnealing(1)
    a["T"] = [(0, T)]
    return a


def _copy(p):
    return {k: np.array(v, copy=True) for k, v in p.items()}


def save(name, **kw):
    np.savez_compressed(os.path.join(HERE, name + ".npz"), **kw)
    print(name, {k: np.shape(v) for k, v in kw.items() if np.ndim(v)})


def step_case(name, model, params, y, T, steps=1, to_learn=None):
    """E_step -> M_step `steps` times; stores the inputs and the last step's outputs (logpj, posteriors_h, params)."""
    p = _copy(params)
    ins = _copy(params)
    for _ in range(steps):
        ins = _copy(p)
        ss = model.E_step(_anneal(T), _copy(p), {"y": y})
        p = model.M_step(_anneal(T), _copy(p), ss, {"y": y})
    kw = {"y": y, "T": T, "D": model.D, "H": model.H, "to_learn": np.array(model.to_learn),
          "logpj": ss["logpj"], "posteriors_h": ss["posteriors_h"]}
    kw.update({"in_" + k: v for k, v in ins.items()})
    kw.update({"out_" + k: v for k, v in p.items()})
    if isinstance(model, MoG):
        kw["sigmas_sq_type"] = model.sigmas_sq_type
    else:
        kw["A"] = model.A
    save("mixture_step_" + name, **kw)


def mog_params(rng, D, H, full, W_scale=1.0):
    W = W_scale * rng.normal(size=(D, H))
    pies = rng.uniform(0.5, 1.5, size=H)
    pies /= pies.sum()
    if full:
        sig = np.empty((H, D, D))
        for h in range(H):
            B = rng.normal(size=(D, D)) / np.sqrt(D)
            sig[h] = 0.5 * np.eye(D) + B @ B.T
    else:
        sig = rng.uniform(0.5, 2.0, size=(H, D))
    return {"W": W, "pies": pies, "sigmas_sq": sig}


def mog_data(rng, p, N, full):
    D, H = p["W"].shape
    s = rng.randint(H, size=N)
    sd = np.sqrt(np.array([p["sigmas_sq"][h].diagonal() for h in range(H)]) if full else p["sigmas_sq"])
    return p["W"].T[s] + sd[s] * rng.normal(size=(N, D))


def single_steps():
    rng = np.random.RandomState(100)
    # MoG diagonal / full, T = 1 and 2, ragged shapes
    for full, tag in ((False, "diag"), (True, "full")):
        D, H, N = (13, 7, 301)
        p = mog_params(rng, D, H, full)
        y = mog_data(rng, p, N, full)
        for T in (1.0, 2.0):
            m = MoG(D, H, sigmas_sq_type="full" if full else "diagonal")
            step_case("mog_%s_T%d" % (tag, T), m, p, y, T)
        m = MoG(D, H, to_learn=["W", "pies"] if not full else ["sigmas_sq", "pies"],
                sigmas_sq_type="full" if full else "diagonal")
        step_case("mog_%s_subset" % tag, m, p, y, 1.0)
        m = MoG(D, H, sigmas_sq_type="full" if full else "diagonal")
        step_case("mog_%s_step2" % tag, m, p, y, 1.5, steps=2)
    # bigger diagonal: H > 64 and D > 64 (several tiles)
    D, H, N = 70, 67, 40
    p = mog_params(rng, D, H, False)
    y = mog_data(rng, p, N, False)
    step_case("mog_diag_big", MoG(D, H, sigmas_sq_type="diagonal"), p, y, 1.0)
    # MoP, A = nan and A = 10 D
    for A, tag in ((np.nan, "nan"), (None, "A")):
        D, H, N = 19, 9, 411
        W = rng.uniform(0.5, 8.0, size=(D, H))
        pies = np.ones(H) / H
        s = rng.randint(H, size=N)
        y = rng.poisson(W.T[s]).astype(np.float64)
        m = MoP(D, H, A=(10 * D if A is None else A))
        step_case("mop_%s" % tag, m, {"W": W, "pies": pies}, y, 1.0)
        step_case("mop_%s_T2" % tag, m, {"W": W, "pies": pies}, y, 2.0)
    D, H, N = 70, 67, 40
    W = rng.uniform(0.5, 8.0, size=(D, H))
    s = rng.randint(H, size=N)
    y = rng.poisson(W.T[s]).astype(np.float64)
    step_case("mop_big", MoP(D, H), {"W": W, "pies": np.ones(H) / H}, y, 1.0)


def clamp_cases():
    rng = np.random.RandomState(200)
    # logpj > 710 (small variances in 100 dimensions: -logdet = 921) next to logpj < -745 (datapoints far from a narrow
    # component)
    D, H, N = 100, 5, 120
    p = mog_params(rng, D, H, False)
    p["sigmas_sq"][0] = 1e-4
    p["sigmas_sq"][1] = 1e-3
    y = mog_data(rng, mog_params(rng, D, H, False), N, False)
    y[:10] = p["W"][:, 0] + 1e-3 * rng.normal(size=(10, D))
    step_case("clamp_mog_big_small", MoG(D, H, sigmas_sq_type="diagonal"), p, y, 1.0)
    D, H, N = 9, 5, 120
    # sigma^2 <= 0 (a zero in one component, a negative in another)
    p = mog_params(rng, D, H, False)
    p["sigmas_sq"][1, 3] = 0.0
    p["sigmas_sq"][2, 0] = -0.5
    y = mog_data(rng, p, N, False)
    step_case("clamp_mog_nonpos", MoG(D, H, sigmas_sq_type="diagonal"), p, y, 1.0)
    # MoP with W <= 0 (a zero and a negative rate), both normalisations
    W = rng.uniform(0.5, 8.0, size=(D, H))
    s = rng.randint(H, size=N)
    y = rng.poisson(W.T[s]).astype(np.float64)
    W[2, 1] = 0.0
    W[4, 3] = -0.25
    step_case("clamp_mop_nonpos", MoP(D, H), {"W": W, "pies": np.ones(H) / H}, y, 1.0)
    step_case("clamp_mop_nonpos_A", MoP(D, H, A=10 * D), {"W": W, "pies": np.ones(H) / H}, y, 1.0)
    # full covariance with an indefinite, non-singular component
    p = mog_params(rng, D, H, True)
    ev, V = np.linalg.eigh(p["sigmas_sq"][2])
    ev[0] = -0.3
    p["sigmas_sq"][2] = (V * ev) @ V.T
    y = mog_data(rng, mog_params(rng, D, H, True), N, True)
    step_case("fallback_mog_full", MoG(D, H, sigmas_sq_type="full"), p, y, 1.0)


def gen_init():
    D, H, N = 25, 10, 64
    out = {}
    W_gt = 10 * generate_bars_dict(H)
    pies_gt = np.arange(1, H + 1) / np.sum(np.arange(1, H + 1))
    for name, model, params in (
            ("mog_diag", MoG(D, H, sigmas_sq_type="diagonal"), {"W": W_gt, "pies": pies_gt,
                                                                 "sigmas_sq": np.ones((H, D)) * 0.5}),
            ("mog_full", MoG(D, H, sigmas_sq_type="full"), {"W": W_gt, "pies": pies_gt,
                                                             "sigmas_sq": np.array([np.eye(D) * 0.7] * H)}),
            ("mop", MoP(D, H), {"W": W_gt, "pies": pies_gt})):
        np.random.seed(3)
        data = model.generate_data(params, N)
        np.random.seed(5)
        init = model.standard_init(data)
        out[name + "_y"] = data["y"]
        out[name + "_s"] = data["s"]
        for k, v in init.items():
            out[name + "_init_" + k] = v
    save("mixture_gen_init", D=D, H=H, N=N, seed_data=3, seed_init=5, W_gt=W_gt, pies_gt=pies_gt, **out)


def trajectory(name, model, params_gt, steps_kept):
    D, H, N, steps = 25, 10, 2000, 20
    np.random.seed(7)
    data = model.generate_data(params_gt, N)
    np.random.seed(11)
    init = model.standard_init(data)
    anneal = LinearAnnealing(steps)
    anneal["T"] = [(0, 2.), (.7, 1.)]
    lp = _copy(init)
    Ws, pies, sigs = [], [], []
    while not anneal.finished:
        new = model.step(anneal, lp, {"y": data["y"]})
        anneal.next(model.gain(lp, new))
        lp = _copy(new)
        Ws.append(lp["W"]); pies.append(lp["pies"])
        if "sigmas_sq" in lp:
            sigs.append(lp["sigmas_sq"])
        if len(Ws) == steps_kept:
            break
    y = data["y"]
    if isinstance(model, MoP):
        assert np.array_equal(y, y.astype(np.uint8))
        y = y.astype(np.uint8)                      # Poisson counts: stored as bytes (the tests read them back as float64)
    elif name == "mog_full":
        assert np.array_equal(y, np.load(os.path.join(HERE, "mixture_traj_mog_diag.npz"))["y"])
        y = np.zeros(0)                             # the same draws as mixture_traj_mog_diag's y (identity covariances)
    kw = dict(D=D, H=H, steps=len(Ws), y=y, W=np.stack(Ws), pies=np.stack(pies))
    kw.update({"init_" + k: v for k, v in init.items()})
    if sigs:
        kw["sigmas_sq"] = np.stack(sigs)
        kw["sigmas_sq_type"] = model.sigmas_sq_type
    else:
        kw["A"] = model.A
    save("mixture_traj_" + name, **kw)


def trajectories():
    D, H = 25, 10
    W_gt = 10 * generate_bars_dict(H)
    pies = 1. / H * np.ones(H)
    trajectory("mog_diag", MoG(D, H, sigmas_sq_type="diagonal"), {"W": W_gt, "pies": pies, "sigmas_sq": np.ones((H, D))},
               20)
    trajectory("mog_full", MoG(D, H, sigmas_sq_type="full"), {"W": W_gt, "pies": pies,
                                                              "sigmas_sq": np.array([np.eye(D)] * H)}, 3)
    trajectory("mop", MoP(D, H), {"W": W_gt, "pies": pies}, 20)
    m = MoP(D, H, A=10 * D)
    trajectory("mop_A", m, {"W": m.normalize(W_gt.T).T, "pies": pies}, 20)


if __name__ == "__main__":
    dlog.ignored = lambda *a, **k: True
    import warnings
    warnings.simplefilter("ignore")
    np.seterr(all="ignore")
    single_steps()
    clamp_cases()
    gen_init()
    trajectories()
