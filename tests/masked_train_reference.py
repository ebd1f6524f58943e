"""NumPy restatement of one BSC EM step on incomplete data, shared by tests/test_masked_train_cpu.py,
tests/test_masked_train_gpu.py and tests/masked_train_world2_gpu_worker.py: the reference's M-step loop (bsc_et.py:332-420)
with the mask m_nd inside every sum over d.  Plain loops over rows and dimensions; an unobserved value is selected away
(np.where), never multiplied.  Not a test module."""
from math import pi as _PI

import numpy as np
from scipy.special import comb, logsumexp

import masked_reference as MR


class Anneal(dict):
    """One annealing point: unknown keys read 0.0 (annealing.py:93-94)."""

    def __missing__(self, key):
        return 0.0

    def as_dict(self):
        return dict(self)


def state_matrix(Hp, gamma):
    from itertools import combinations
    rows = [s for g in range(2, gamma + 1) for s in combinations(range(Hp), g)]
    SM = np.zeros((len(rows), Hp), dtype=np.uint8)
    for i, s in enumerate(rows):
        SM[i, list(s)] = 1
    return SM


def pi_gamma_factors(pies, H, gamma):
    A = B = 0
    for g in range(gamma + 1):
        t = comb(H, g) * (pies ** g) * ((1 - pies) ** (H - g))
        A += t
        B += g * t
    return A, B, pies * H * A / B


def pair_list(Hp):
    return [(i, j) for i in range(Hp) for j in range(i + 1, Hp)]


def e_step(anneal, params, Y, M, Hp, SM):
    """Selection and log-joints of the masked E-step at the annealing point: (cand (N, H'), logpj (N, 1+H+S), e (N, K) the
    masked energies, size (N, K), dict of the dense terms)."""
    W = np.asarray(params["W"], dtype=np.float64)
    D, H = W.shape
    mu = np.asarray(params.get("mu", np.zeros(D)), dtype=np.float64)
    Mb = np.asarray(M) != 0
    X = np.where(Mb, np.asarray(Y, dtype=np.float64) - mu[None, :], 0.0)
    Mf = Mb.astype(np.float64)
    b, g, xn2 = X @ W, Mf @ (W * W), (X * X).sum(axis=1)
    cand = MR.bsc_select_rule(b, g, Hp)
    size, e = MR.bsc_masked_terms(b, g, xn2, Mb, W.T, cand, SM)
    pies, sigma = float(params["pi"]), float(params["sigma"])
    beta = 1. / anneal["T"]
    ecoef = beta * (-0.5 / sigma / sigma)
    ppil = (beta if anneal["anneal_prior"] else 1.0) * np.log(pies / (1. - pies))
    return cand, ppil * size + ecoef * e, e, size, {"X": X, "Mf": Mf, "b": b, "g": g, "dn": Mb.sum(axis=1)}


def row_stats(logpj, e, cand, SM, H):
    """Per row: E[s] (N, H), the candidates' pair moments q2 (N, H'(H'-1)/2) in the order (0,1), (0,2), ..., the expected
    energy (N,) and the log-sum-exp (N,)."""
    N = logpj.shape[0]
    Hp = cand.shape[1]
    SMf = np.asarray(SM, dtype=np.float64)
    lse = logsumexp(logpj, axis=1) if N else np.zeros(0)
    q = np.exp(logpj - lse[:, None])
    qs = q[:, 1 + H:]
    Es = q[:, 1:1 + H].copy()
    np.add.at(Es, (np.arange(N)[:, None], cand), qs @ SMf)
    pairs = pair_list(Hp)
    q2 = np.zeros((N, len(pairs)))
    for p, (i, j) in enumerate(pairs):
        q2[:, p] = qs[:, (SMf[:, i] > 0) & (SMf[:, j] > 0)].sum(axis=1)
    with np.errstate(invalid="ignore"):
        energy = np.where(q > 0, q * e, 0.0).sum(axis=1)
    return Es, q2, energy, lse


def pair_tensor(cand, q2, Mb, diagT, H):
    """A (D, H, H): A[d, c_i, c_j] = A[d, c_j, c_i] = sum_n m_nd q2[n, (i,j)], every cell added in ascending n; the diagonal
    from ``diagT`` (D, H)."""
    N, Hp = cand.shape
    D = Mb.shape[1]
    A = np.zeros((D, H, H))
    pairs = pair_list(Hp)
    for n in range(N):
        obs = np.nonzero(Mb[n])[0]
        if not obs.size:
            continue
        Q = np.zeros((Hp, Hp))
        for p, (i, j) in enumerate(pairs):
            Q[i, j] = Q[j, i] = q2[n, p]
        c = cand[n]
        A[obs[:, None, None], c[None, :, None], c[None, None, :]] += Q[None]
    idx = np.arange(H)
    A[:, idx, idx] = diagT
    return A


def solve_ok(piv_min, piv_max):
    ratio = piv_min / piv_max if piv_max != 0 else 0.0
    return piv_min > 0 and np.isfinite(ratio) and ratio > 1e-11


def solve_rows(A, r, W_old):
    """W_new (D, H): row d solves A_d w = r[:, d] where the system is usable (positive pivots, ratio above 1e-11), else keeps
    its old row.  Returns (W_new, kept (D,) bool)."""
    D, H = W_old.shape
    W_new = np.array(W_old, dtype=np.float64, copy=True)
    kept = np.ones(D, dtype=bool)
    for d in range(D):
        try:
            piv = np.diag(np.linalg.cholesky(A[d])) ** 2
        except np.linalg.LinAlgError:
            continue
        if not solve_ok(piv.min(), piv.max()):
            continue
        W_new[d] = np.linalg.solve(A[d], r[:, d])
        kept[d] = False
    return W_new, kept


def statistics(anneal, params, Y, M, Hp, gamma):
    """Everything one shard contributes: a dict with cand, logpj, lse, Es, q2, energy, A, r and the packed totals."""
    W = np.asarray(params["W"], dtype=np.float64)
    D, H = W.shape
    SM = state_matrix(Hp, gamma)
    cand, logpj, e, size, dense = e_step(anneal, params, Y, M, Hp, SM)
    Es, q2, energy, lse = row_stats(logpj, e, cand, SM, H)
    Mb = np.asarray(M) != 0
    A = pair_tensor(cand, q2, Mb, dense["Mf"].T @ Es, H)
    r = Es.T @ dense["X"]
    return {"cand": cand, "logpj": logpj, "lse": lse, "Es": Es, "q2": q2, "energy": energy, "A": A, "r": r,
            "sumE": Es.sum(axis=0), "sum_energy": energy.sum(), "sum_lse": lse.sum(), "N": Y.shape[0],
            "sum_dn": int(dense["dn"].sum()), "e": e}


def step(anneal, params, Y, M, Hp, gamma, to_learn=("W", "pi", "sigma"), shards=None):
    """One masked EM step.  ``shards``: list of row-index arrays, the statistics are formed per shard and added (the
    all-reduce).  Returns (new parameters, log dict: L, N, kept, W_kept and the first shard's per-row statistics)."""
    W = np.asarray(params["W"], dtype=np.float64)
    D, H = W.shape
    pies, sigma = float(params["pi"]), float(params["sigma"])
    Y, M = np.asarray(Y), np.asarray(M)
    if shards is None:
        shards = [np.arange(Y.shape[0])]
    parts = [statistics(anneal, params, Y[s], M[s], Hp, gamma) for s in shards]
    tot = {k: sum(p[k] for p in parts) for k in ("A", "r", "sumE", "sum_energy", "sum_lse", "N", "sum_dn")}
    A_pg, _, E_pg = pi_gamma_factors(pies, H, gamma)
    N = tot["N"]
    if "W" in to_learn:
        W_new, kept = solve_rows(tot["A"], tot["r"], W)
    else:
        W_new, kept = W.copy(), np.zeros(D, dtype=bool)
    pi_new = E_pg * tot["sumE"].sum() / H / N if "pi" in to_learn else pies
    sigma_new = np.sqrt(tot["sum_energy"] / tot["sum_dn"]) if "sigma" in to_learn else sigma
    c0, c1 = H * np.log(1. - pies), -0.5 * np.log(2 * _PI * sigma ** 2)
    L = (N * c0 + tot["sum_dn"] * c1 + tot["sum_lse"]) / N - np.log(A_pg)
    new = {"W": W_new, "pi": pi_new, "sigma": sigma_new,
           "mu": np.asarray(params.get("mu", np.zeros(D)), dtype=np.float64)}
    log = dict(parts[0])
    log.update({"L": L, "N": N, "kept": kept, "W_kept": int(kept.sum()), "tot": tot})
    return new, log


# ------------------------------------------------------------------------------------------------------- test problems
def bars_problem(rng, p=4, N=300, pi=0.2, sigma=1.0, height=5.0, frac=0.6):
    """Bars data (p x p pixels, 2p bars) with ``1 - frac`` of the entries missing; row 0 fully observed, row 1 not at all."""
    D, H = p * p, 2 * p
    W = np.zeros((D, H))
    for k in range(p):
        img = np.zeros((p, p))
        img[k, :] = height
        W[:, k] = img.ravel()
        img = np.zeros((p, p))
        img[:, k] = height
        W[:, p + k] = img.ravel()
    S = rng.uniform(size=(N, H)) < pi
    Y = S @ W.T + sigma * rng.normal(size=(N, D))
    M = rng.uniform(size=(N, D)) < frac
    M[0] = True
    M[1] = False
    return W, Y, M


def model_problem(rng, D, H, N, frac=0.5, sigma=1.0, never=True, pi=None):
    """Data drawn from the model, parameters near the generating ones, ``frac`` observed with row 0 fully observed, row 1
    unobserved and (``never``) the last dimension never observed.  Every other row keeps at least two observed dimensions
    (with one, every selection score is +-x_d: exact ties).  ``pi`` defaults to what gives every latent about 12 observed
    active rows per dimension (well-conditioned per-dimension normal matrices) while a row's active latents still fit
    into the candidates used with these shapes (H' >= 0.3 H or >= 4)."""
    if pi is None:
        pi = min(0.45, max(2.0 / H, 12.0 / (N * frac)), max(2.8 / H, 0.2))
    W_gt = rng.normal(size=(D, H)) * 3.0
    S = rng.uniform(size=(N, H)) < pi
    Y = S @ W_gt.T + sigma * rng.normal(size=(N, D))
    M = rng.uniform(size=(N, D)) < frac
    if never and D > 1:
        M[:, D - 1] = False
    Dl = D - 1 if never and D > 1 else D
    for n in np.nonzero(M.sum(axis=1) < 2)[0]:
        M[n, rng.choice(Dl, min(2, Dl), replace=False)] = True
    M[0] = True
    if N > 1:
        M[1] = False
    if never and D > 1:
        M[:, D - 1] = False
    params = {"W": W_gt + 0.05 * rng.normal(size=(D, H)), "pi": pi * 1.1, "sigma": sigma * 1.1}
    return params, Y, M


def conditioning(log, M):
    """Largest cond(A_d) over the dimensions somebody observed."""
    obs = (np.asarray(M) != 0).any(axis=0)
    return max(np.linalg.cond(log["tot"]["A"][d]) for d in np.nonzero(obs)[0])


def exact_em_start():
    """The exact-EM problem (H' = gamma = H = 8, D = 16, N = 300, 40 % missing, one row unobserved, one fully observed):
    (start parameters, Y with NaN holes, mask)."""
    rng = np.random.RandomState(11)
    W_gt, Y, M = bars_problem(rng)
    D, H = W_gt.shape
    params = {"W": W_gt + rng.normal(size=(D, H)), "pi": 0.3, "sigma": 2.0}
    return params, np.where(M, Y, np.nan), M


_TRAJ = {}


def exact_em_trajectory(steps=25):
    """The NumPy trajectory from ``exact_em_start``: (list of L, final parameters); computed once."""
    if steps not in _TRAJ:
        params, Yh, M = exact_em_start()
        H = params["W"].shape[1]
        an = Anneal(T=1.0)
        Ls = []
        for _ in range(steps):
            params, log = step(an, params, Yh, M, H, H)
            Ls.append(log["L"])
        _TRAJ[steps] = (Ls, params)
    return _TRAJ[steps]
