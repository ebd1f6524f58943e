"""Mixture models (MoG diagonal / full, MoP with and without normalisation) on the MI355X against the reference's own
outputs (tests/golden/mixture_*.npz, make_golden_mixture.py) and, at benchmark size, against a float64 NumPy
restatement written out below."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden

pytestmark = pytest.mark.gpu

TINY = np.finfo(np.float64).tiny
EPS = np.finfo(np.float64).eps


class An(dict):
    def __missing__(self, k):
        return 0.0

    def as_dict(self):
        return dict(self)


def _model(g):
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.em.mixturemodels.MoP import MoP
    D, H = int(g["D"]), int(g["H"])
    to_learn = [str(x) for x in g["to_learn"]] if "to_learn" in g else None
    if "sigmas_sq_type" in g:
        kw = {"sigmas_sq_type": str(g["sigmas_sq_type"])}
        return MoG(D, H, to_learn=to_learn, **kw) if to_learn else MoG(D, H, **kw)
    A = float(g["A"])
    return MoP(D, H, to_learn=to_learn, A=A) if to_learn else MoP(D, H, A=A)


def _params(g, prefix):
    return {k[len(prefix):]: np.array(v) for k, v in g.items() if k.startswith(prefix)}


def _expanded_scale(g):
    """|logpj| error scale of the expanded MoG form: sum_d (y^2 + w^2) / sigma^2 per (n, h), times beta."""
    if "sigmas_sq_type" not in g or str(g["sigmas_sq_type"]) != "diagonal":
        return None
    sig = g["in_sigmas_sq"]
    with np.errstate(all="ignore"):
        return ((g["y"] ** 2) @ (1 / sig).T + np.sum(g["in_W"].T ** 2 / sig, 1)[None, :]) / float(g["T"])


STEP_CASES = sorted(os.path.basename(p)[len("mixture_step_"):-4] for p in glob.glob(os.path.join(GOLDEN, "mixture_step_*.npz")))


@pytest.mark.parametrize("case", STEP_CASES)
def test_single_step_golden(case):
    g = golden("mixture_step_%s.npz" % case)
    m = _model(g)
    params = _params(g, "in_")
    ss = m.E_step(An(T=float(g["T"])), {k: v.copy() for k, v in params.items()}, {"y": g["y"]})
    lp, post = np.asarray(ss["logpj"]), np.asarray(ss["posteriors_h"])
    ref = g["logpj"]
    # the same non-finite pattern as the reference, element for element (IEEE inf / NaN through the MFMA path)
    np.testing.assert_array_equal(np.isnan(lp), np.isnan(ref))
    np.testing.assert_array_equal(np.isposinf(lp), np.isposinf(ref))
    np.testing.assert_array_equal(np.isneginf(lp), np.isneginf(ref))
    fin = np.isfinite(ref)
    scale = _expanded_scale(g)
    atol = 1e-13 * (scale[fin] if scale is not None else np.abs(ref[fin]).max(initial=1.0))
    # rtol 1e-10, and 1e-8 for a component that took the host inverse (an indefinite covariance: its quadratic form is
    # ill-conditioned)
    rtol = np.full(ref.shape, 1e-10)
    rtol[:, getattr(m, "fallback_components", [])] = 1e-8
    assert np.all(np.abs(lp[fin] - ref[fin]) <= rtol[fin] * np.abs(ref[fin]) + atol), np.abs(lp[fin] - ref[fin]).max()
    np.testing.assert_allclose(post, g["posteriors_h"], rtol=0, atol=1e-12)
    new = m.M_step(An(T=float(g["T"])), {k: v.copy() for k, v in params.items()}, ss, {"y": g["y"]})
    out = _params(g, "out_")
    assert sorted(new) == sorted(out)
    for k in out:
        np.testing.assert_allclose(new[k], out[k], rtol=1e-8 if case.startswith("fallback") else 1e-9,
                                   atol=1e-12 * max(1.0, np.abs(out[k]).max()), err_msg=k)


@pytest.mark.parametrize("case", [c for c in STEP_CASES if "full" in c])
def test_full_covariance_fallback_only_where_cholesky_fails(case):
    """The device Cholesky factors every positive definite covariance; only the indefinite component of the fallback
    fixture (index 2) takes the host inverse, and the other components match the reference at rtol 1e-10."""
    g = golden("mixture_step_%s.npz" % case)
    m = _model(g)
    params = _params(g, "in_")
    ss = m.E_step(An(T=float(g["T"])), {k: v.copy() for k, v in params.items()}, {"y": g["y"]})
    assert m.fallback_components == ([2] if case.startswith("fallback") else [])
    ok = [h for h in range(int(g["H"])) if h not in m.fallback_components]
    np.testing.assert_allclose(np.asarray(ss["logpj"])[:, ok], g["logpj"][:, ok], rtol=1e-10)


@pytest.mark.parametrize("case", ["mop_A", "mop_nan", "clamp_mop_nonpos_A"])
def test_mop_posterior_takes_model_data_as_the_reference(case):
    """MoP.posterior / log_p_y take the data as the reference's do (normalised by the caller when A is set,
    MoP.py:93-103) and log_p_y returns an ndarray."""
    g = golden("mixture_step_%s.npz" % case)
    m = _model(g)
    params = _params(g, "in_")
    y = g["y"] if np.isnan(m.A) else m.normalize(g["y"])
    out = m.posterior({k: v.copy() for k, v in params.items()}, y, 1. / float(g["T"]))
    ref = g["logpj"]
    lp = np.asarray(out["logpj"])
    np.testing.assert_array_equal(np.isfinite(lp), np.isfinite(ref))
    fin = np.isfinite(ref)
    np.testing.assert_allclose(lp[fin], ref[fin], rtol=1e-10, atol=1e-10 * np.abs(ref[fin]).max())
    np.testing.assert_allclose(np.asarray(out["posteriors_h"]), g["posteriors_h"], atol=1e-12)
    lpy = m.log_p_y({k: v.copy() for k, v in params.items()}, y, 1. / float(g["T"]))
    assert isinstance(lpy, np.ndarray) and lpy.shape == ref.shape


@pytest.mark.parametrize("name", ["mog_diag", "mog_full", "mop", "mop_A"])
def test_trajectory_golden(name):
    from prosper_amd.em.annealing import LinearAnnealing
    g = golden("mixture_traj_%s.npz" % name)
    y = g["y"].astype(np.float64) if g["y"].size else golden("mixture_traj_mog_diag.npz")["y"]
    if name == "mog_full":
        g["sigmas_sq_type"] = "full"
    m = _model(dict(g, **({"A": g["A"]} if "A" in g else {})))
    anneal = LinearAnnealing(20)
    anneal["T"] = [(0, 2.), (.7, 1.)]
    p = {k: v.copy() for k, v in _params(g, "init_").items()}
    for step in range(int(g["steps"])):
        p = m.step(anneal, p, {"y": y})
        anneal.next(0.)
        for k in ("W", "pies", "sigmas_sq"):
            if k in g:
                ref = g[k][step]
                assert np.abs(p[k] - ref).max() <= 1e-10 * np.abs(ref).max(), (step, k, np.abs(p[k] - ref).max())
        p = {k: np.array(v, copy=True) for k, v in p.items()}


# ---- at size, against a float64 NumPy restatement --------------------------------------------------------------------
def np_posterior(logpj, H):
    with np.errstate(all="ignore"):
        p = np.exp(logpj)
    p[np.isnan(p)] = TINY
    p[p < TINY] = TINY
    p[np.isinf(p)] = np.finfo(np.float64).max / H
    return p / p.sum(1)[:, None]


def np_logpj_diag(y, W, sig, pies, beta):
    out = np.empty((y.shape[0], W.shape[1]))
    for h in range(W.shape[1]):
        u = y - W[:, h]
        out[:, h] = -(np.sum(np.log(sig[h])) + np.sum(u * u / sig[h], 1)) * beta
    return out + np.log(pies) * beta


def np_logpj_full(y, W, sig, pies, beta):
    out = np.empty((y.shape[0], W.shape[1]))
    for h in range(W.shape[1]):
        u = y - W[:, h]
        out[:, h] = -(np.linalg.slogdet(sig[h])[1] + np.sum((u @ np.linalg.inv(sig[h])) * u, 1)) * beta
    return out + np.log(pies) * beta


def np_logpj_mop(y, W, pies, beta):
    return (y @ np.log(W) - W.sum(0)[None, :]) * beta + np.log(pies) * beta


@pytest.fixture(scope="module")
def big():
    rng = np.random.RandomState(5)
    N, D, H = 200000, 1024, 256
    W = rng.uniform(1.0, 3.0, size=(D, H))
    s = rng.randint(H, size=N)
    y = (W.T[s] + rng.normal(size=(N, D)) * 0.5)
    return {"N": N, "D": D, "H": H, "W": W, "y": y, "rows": rng.choice(N, 512, replace=False)}


@pytest.mark.timeout(600)
@pytest.mark.parametrize("kind", ["mog_diag", "mop"])
def test_one_step_at_size(big, kind):
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.em.mixturemodels.MoP import MoP
    N, D, H, y, rows = big["N"], big["D"], big["H"], big["y"], big["rows"]
    rng = np.random.RandomState(9)
    pies = rng.uniform(0.5, 1.5, H)
    pies /= pies.sum()
    W = big["W"] + 0.1 * rng.normal(size=(D, H))
    beta = 1 / 1.3
    if kind == "mop":
        y = np.floor(np.abs(y) * 2)
        m, params = MoP(D, H), {"W": W, "pies": pies}
        ref_lp = np_logpj_mop(y[rows], W, pies, beta)
        tol = 1e-10 * np.abs(ref_lp).max()
    else:
        sig = rng.uniform(0.5, 1.5, (H, D))
        m, params = MoG(D, H, sigmas_sq_type="diagonal"), {"W": W, "pies": pies, "sigmas_sq": sig}
        ref_lp = np_logpj_diag(y[rows], W, sig, pies, beta)
        tol = 1e-13 * (((y[rows] ** 2) @ (1 / sig).T) + np.sum(W.T ** 2 / sig, 1)).max()
    ss = m.E_step(An(T=1.3), dict(params), {"y": y})
    lp = ss["logpj"].tensor[rows].cpu().numpy()
    post = ss["posteriors_h"].tensor[rows].cpu().numpy()
    assert np.abs(lp - ref_lp).max() <= tol + 1e-10 * np.abs(ref_lp).max()
    np.testing.assert_allclose(post, np_posterior(ref_lp, H), atol=1e-10)
    P = np.asarray(ss["posteriors_h"])
    new = m.M_step(An(T=1.3), dict(params), ss, {"y": y})
    cs = P.sum(0)
    if kind == "mop":
        W_ref = (y.T @ P) / cs[None, :] + EPS
        np.testing.assert_allclose(new["W"], W_ref, rtol=1e-9)
    else:
        sp = cs + TINY
        W_ref = (y.T @ P) / sp[None, :]
        sig_ref = ((y ** 2).T @ P).T / sp[:, None] - W_ref.T ** 2
        np.testing.assert_allclose(new["W"], W_ref, rtol=1e-9)
        np.testing.assert_allclose(new["sigmas_sq"], sig_ref, rtol=1e-9, atol=1e-9 * np.abs(sig_ref).max())
    np.testing.assert_allclose(new["pies"], (cs + TINY) / (cs + TINY).sum(), rtol=1e-9)


@pytest.mark.timeout(600)
def test_full_covariance_at_size():
    from prosper_amd.em.mixturemodels.MoG import MoG
    rng = np.random.RandomState(6)
    N, D, H = 50000, 128, 64
    W = rng.normal(size=(D, H))
    s = rng.randint(H, size=N)
    y = W.T[s] + rng.normal(size=(N, D))
    sig = np.empty((H, D, D))
    for h in range(H):
        B = rng.normal(size=(D, D)) / np.sqrt(D)
        sig[h] = np.eye(D) + 0.3 * B @ B.T
    pies = np.ones(H) / H
    m = MoG(D, H, sigmas_sq_type="full")
    params = {"W": W + 0.05 * rng.normal(size=(D, H)), "pies": pies, "sigmas_sq": sig}
    rows = rng.choice(N, 256, replace=False)
    ss = m.E_step(An(T=1.0), dict(params), {"y": y})
    ref_lp = np_logpj_full(y[rows], params["W"], sig, pies, 1.0)
    lp = ss["logpj"].tensor[rows].cpu().numpy()
    np.testing.assert_allclose(lp, ref_lp, rtol=1e-10, atol=1e-10 * np.abs(ref_lp).max())
    np.testing.assert_allclose(ss["posteriors_h"].tensor[rows].cpu().numpy(), np_posterior(ref_lp, H), atol=1e-10)
    P = np.asarray(ss["posteriors_h"])
    new = m.M_step(An(T=1.0), dict(params), ss, {"y": y})
    sp = P.sum(0) + TINY
    W_ref = (y.T @ P) / sp[None, :]
    np.testing.assert_allclose(new["W"], W_ref, rtol=1e-9, atol=1e-12)
    for h in (0, 17, H - 1):
        G = (y * P[:, h:h + 1]).T @ y / sp[h] - np.outer(W_ref[:, h], W_ref[:, h])
        np.testing.assert_allclose(new["sigmas_sq"][h], G, rtol=1e-9, atol=1e-9 * np.abs(G).max())


# ---- repeatability, foreign posteriors, partial data, two ranks ----------------------------------------------------------
@pytest.mark.parametrize("case", ["mog_diag_big", "mog_full_T1", "mop_A", "mop_big"])
def test_repeatable_and_foreign_posteriors(case):
    g = golden("mixture_step_%s.npz" % case)
    m = _model(g)
    params = _params(g, "in_")
    runs = []
    for _ in range(2):
        ss = m.E_step(An(T=float(g["T"])), {k: v.copy() for k, v in params.items()}, {"y": g["y"]})
        new = m.M_step(An(T=float(g["T"])), {k: v.copy() for k, v in params.items()}, ss, {"y": g["y"]})
        runs.append((np.asarray(ss["logpj"]).copy(), np.asarray(ss["posteriors_h"]).copy(), new))
    assert np.array_equal(runs[0][0], runs[1][0], equal_nan=True)
    assert np.array_equal(runs[0][1], runs[1][1])
    for k in runs[0][2]:
        assert np.array_equal(runs[0][2][k], runs[1][2][k]), k
    # NumPy posteriors (e.g. a user's) into M_step: the same result as the device handle
    foreign = m.M_step(An(T=float(g["T"])), {k: v.copy() for k, v in params.items()},
                       {"posteriors_h": runs[0][1].copy()}, {"y": g["y"].copy()})
    for k in foreign:
        assert np.array_equal(foreign[k], runs[0][2][k]), k


def test_partial_data_step():
    g = golden("mixture_step_mop_big.npz")
    m = _model(g)
    params = _params(g, "in_")
    np.random.seed(1)
    new = m.step(An(T=1.0, partial=0.5), {k: v.copy() for k, v in params.items()}, {"y": g["y"]})
    np.random.seed(1)
    sel = np.random.permutation(g["y"].shape[0])[:int(np.ceil(g["y"].shape[0] * 0.5))]
    ss = m.E_step(An(T=1.0), {k: v.copy() for k, v in params.items()}, {"y": g["y"][sel]})
    ref = m.M_step(An(T=1.0), {k: v.copy() for k, v in params.items()}, ss, {"y": g["y"][sel]})
    for k in ref:
        assert np.array_equal(new[k], ref[k]), k


@pytest.mark.timeout(600)
def test_two_ranks_over_gloo():
    """Two processes on the one GPU, a world_size-2 gloo group (tests/mixture_world2_gpu_worker.py): bitwise identical
    parameters on both ranks after every step, and the single-rank step within rounding."""
    import socket
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    procs = []
    for rank in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2",
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "mixture_world2_gpu_worker.py")],
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=500))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for rank, (p, (out, err)) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and ("ok %d" % rank) in out.split("\n"), "rank %d\n%s\n%s" % (rank, out[-2000:], err[-4000:])
