"""Exact EM for the linear models by plain NumPy enumeration: every state of {values}^H, one row at a time.

  moments(Y, W, sigma, values, logp, mu)   per row E[s], E[s s^T] packed as (0,0), (0,1), ..., (0,H-1), (1,1), ... and
                                           v_n = log sum_s exp l_n(s), l_n(s) = sum_h logp[h, k_h] - 1/2 s^T G s + s^T B_n,
                                           G = W^T W / sigma^2, B_n = W^T (y_n - mu) / sigma^2 (pm_moments_exact_lin_f64)
  step(anneal, params, Y, to_learn)        one exact BSC EM step: the reference's M-step at H' = gamma = H (A_pi_gamma =
                                           E_pi_gamma = 1), annealed as its E-step is
"""
import itertools

import numpy as np


class Anneal(dict):
    """One annealing point: unknown keys read 0.0 (annealing.py:93-94)."""

    def __missing__(self, key):
        return 0.0

    def as_dict(self):
        return dict(self)


def states(values, H):
    values = np.asarray(values, dtype=np.float64)
    idx = np.array(list(itertools.product(range(len(values)), repeat=H)), dtype=np.int64).reshape(-1, H)
    return idx, values[idx]


def pair_index(H):
    return np.triu_indices(H)


def moments(Y, W, sigma, values, logp, mu=None):
    Y = np.asarray(Y, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    N, D = Y.shape
    H = W.shape[1]
    idx, S = states(values, H)
    logp = np.asarray(logp, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        prior = logp[np.arange(H)[None, :], idx].sum(axis=1)
    G = W.T @ W / sigma ** 2
    quad = -0.5 * np.einsum("sh,hk,sk->s", S, G, S)
    iu = pair_index(H)
    SS = S[:, iu[0]] * S[:, iu[1]]
    E = np.zeros((N, H))
    C = np.zeros((N, len(iu[0])))
    v = np.zeros(N)
    for n in range(N):
        x = Y[n] - (0.0 if mu is None else np.asarray(mu, dtype=np.float64))
        B = W.T @ x / sigma ** 2
        l = prior + quad + S @ B
        if not np.all(np.isfinite(x)):
            E[n], C[n], v[n] = np.nan, np.nan, np.nan
            continue
        m = l.max()
        w = np.exp(l - m)
        z = w.sum()
        q = w / z
        v[n] = m + np.log(z)
        E[n] = q @ S
        C[n] = q @ SS
    return E, C, v


def step(anneal, params, Y, to_learn=("W", "pi", "sigma"), shards=None):
    """Returns (new parameters, log): log carries N, L, N_use, the totals (Wp against y - mu, Wq, mus, energy, Fs) and the
    condition number of Wq.  ``shards``: lists of rows whose statistics are formed apart and added."""
    Y = np.asarray(Y, dtype=np.float64)
    W = np.asarray(params["W"], dtype=np.float64)
    N, D = Y.shape
    H = W.shape[1]
    pi, sigma = float(params["pi"]), float(params["sigma"])
    mu = np.asarray(params.get("mu", np.zeros(D)), dtype=np.float64)
    beta = 1.0 / anneal["T"]
    odds = (beta if anneal["anneal_prior"] else 1.0) * np.log(pi / (1.0 - pi))
    idx, S = states([0.0, 1.0], H)
    tot = None
    for rows in (shards if shards is not None else [np.arange(N)]):
        st = {"Wp": np.zeros((H, D)), "Wq": np.zeros((H, H)), "mus": np.zeros(H), "energy": 0.0, "Fs": 0.0,
              "data_sum": np.zeros(D)}
        for n in rows:
            x = Y[n] - mu
            e = ((x[None, :] - S @ W.T) ** 2).sum(axis=1)
            l = odds * S.sum(axis=1) - 0.5 * beta * e / sigma ** 2
            m = l.max()
            w = np.exp(l - m)
            q = w / w.sum()
            es = q @ S
            st["Fs"] += m + np.log(w.sum())
            st["mus"] += es
            st["Wp"] += np.outer(es, x)
            st["Wq"] += (S * q[:, None]).T @ S
            st["energy"] += q @ e
            st["data_sum"] += Y[n]
        tot = st if tot is None else {k: tot[k] + st[k] for k in tot}
    W_new = np.linalg.solve(tot["Wq"], tot["Wp"]) if "W" in to_learn else W.T
    pi_new = tot["mus"].sum() / H / N if "pi" in to_learn else pi
    sigma_new = np.sqrt(tot["energy"] / D / N) if "sigma" in to_learn else sigma
    mu_new = tot["data_sum"] / N - np.inner(W_new.T / N, tot["mus"]) if "mu" in to_learn else mu
    L = H * np.log(1.0 - pi) - 0.5 * D * np.log(2 * np.pi * sigma ** 2) + tot["Fs"] / N
    log = {"N": N, "N_use": N, "L": L, "stats": tot, "cond": float(np.linalg.cond(tot["Wq"]))}
    return {"W": W_new.T, "pi": pi_new, "sigma": sigma_new, "mu": mu_new}, log


def problem(rng, D, H, N, pi=None, sigma=0.6, mu=False, scale=3.0):
    """Data drawn from a BSC model and start parameters near the generating dictionary, so that sum_n E[s s^T] is well
    conditioned."""
    pi = 2.0 / H if pi is None else pi
    Wg = scale * rng.normal(size=(D, H))
    s = (rng.random_sample((N, H)) < pi).astype(np.float64)
    m = rng.normal(size=D) if mu else np.zeros(D)
    Y = s @ Wg.T + m + sigma * rng.normal(size=(N, D))
    params = {"W": Wg + 0.1 * rng.normal(size=(D, H)), "pi": 1.1 * pi, "sigma": 1.1 * sigma}
    if mu:
        params["mu"] = m + 0.05 * rng.normal(size=D)
    return params, Y
