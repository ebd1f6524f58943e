"""NumPy restatements of reconstruct(), shared by tests/test_reconstruct_cpu.py and
tests/test_reconstruct_gpu.py: the posterior mean by plain enumeration of every state with the proper densities, and the
same sum over a truncated state set rebuilt from an E-step's (logpj, candidates); its two parts on their own
(expect_from_lpj, mca_multi_from_lpj) are what tests/test_eval_kernels_gpu.py holds the two kernels to.  Not a test module."""
import itertools

import numpy as np
from scipy.special import logsumexp


def softmax_rows(Z):
    """exp(Z - rowLSE): NaN rows stay NaN, -inf entries give 0."""
    with np.errstate(invalid="ignore"):
        return np.exp(Z - logsumexp(Z, axis=1, keepdims=True))


# ---------------------------------------------------------------------------------------------------------- enumeration
def enum_states(values, H):
    return np.array(list(itertools.product(list(values), repeat=H)), dtype=np.float64)


def enum_mean(Y, means, log_prior, var):
    """sum_s p(s | y_n) means[s] for y ~ N(means[s], var I): (N, D)."""
    r2 = ((Y[:, None, :] - means[None, :, :]) ** 2).sum(-1)
    with np.errstate(invalid="ignore"):
        q = softmax_rows(log_prior[None, :] - 0.5 * r2 / var)
    return q @ means


def enum_linear(Y, W, sigma, values, logp, mu=None):
    """BSC / DSC / TSC: states values^H, log prior sum_h logp[k_h], mean mu + W s."""
    H = W.shape[1]
    values = np.asarray(values, dtype=np.float64)
    idx = np.array(list(itertools.product(range(len(values)), repeat=H)))
    S = values[idx]
    with np.errstate(invalid="ignore"):
        lp = np.asarray(logp, dtype=np.float64)[idx].sum(axis=1)
    keep = np.isfinite(lp)                       # a state of zero prior contributes nothing
    means = S[keep] @ W.T + (0.0 if mu is None else np.asarray(mu)[None, :])
    return enum_mean(Y, means, lp[keep], sigma ** 2)


def mca_mean(W, rho, signed):
    def mean(active):
        active = np.asarray(active, dtype=int)
        if not active.size:
            return np.zeros(W.shape[0])
        Wa = W[:, active]
        if signed:
            t = (np.sign(Wa) * np.abs(Wa) ** rho).sum(axis=1)
            return np.sign(t) * np.abs(t) ** (1. / rho)
        return ((Wa ** rho).sum(axis=1)) ** (1. / rho)
    return mean


def enum_mca(Y, W, rho, signed, pi, sigma):
    H = W.shape[1]
    S = enum_states([0, 1], H)
    mean = mca_mean(W, rho, signed)
    means = np.array([mean(np.nonzero(s)[0]) for s in S])
    lp = S.sum(1) * np.log(pi) + (H - S.sum(1)) * np.log(1 - pi)
    return enum_mean(Y, means, lp, sigma ** 2)


def _gsc_sigma(p, D):
    sig = np.asarray(p["sigma_sq"], dtype=np.float64)
    return sig * np.eye(D) if sig.ndim == 0 else (np.diag(sig) if sig.ndim == 1 else sig)


def gsc_state_terms(p, Y, active):
    """(log p(s, y_n) up to a constant common to all states, W_s E[z_s | s, y_n]) of the support ``active``."""
    W, mu, Psi = p["W"], np.asarray(p["mu"], dtype=np.float64), p["psi_sq"]
    D, H = W.shape
    pi = np.broadcast_to(np.asarray(p["pi"], dtype=np.float64), (H,))
    Sig = _gsc_sigma(p, D)
    a = np.asarray(active, dtype=int)
    lp = np.log(pi[a]).sum() + np.log(1 - np.delete(pi, a)).sum()
    Wa = W[:, a]
    Pa = Psi[np.ix_(a, a)]
    C = Sig + Wa @ Pa @ Wa.T
    r = Y - (Wa @ mu[a])[None, :]
    _, ld = np.linalg.slogdet(C)
    Cr = np.linalg.solve(C, r.T)                                  # (D, N)
    logp = lp - 0.5 * ld - 0.5 * (r * Cr.T).sum(axis=1)
    kappa = mu[a][None, :] + (Pa @ Wa.T @ Cr).T                   # (N, |a|)
    return logp, kappa @ Wa.T


def enum_gsc(p, Y):
    H = p["W"].shape[1]
    sets = [np.nonzero(s)[0] for s in itertools.product([0, 1], repeat=H)]
    return gsc_from_sets(p, Y, [sets] * len(Y))


def gsc_from_sets(p, Y, sets_per_row):
    """sum over each row's own list of supports.  Rows that share the same list object are evaluated together."""
    out = np.empty_like(Y)
    groups = {}
    for n, sets in enumerate(sets_per_row):
        groups.setdefault(id(sets), (sets, []))[1].append(n)
    for sets, rows in groups.values():
        rows = np.array(rows)
        terms = [gsc_state_terms(p, Y[rows], a) for a in sets]
        q = softmax_rows(np.stack([t[0] for t in terms], axis=1))
        out[rows] = sum(q[:, k:k + 1] * terms[k][1] for k in range(len(sets)))
    return out


# ---------------------------------------------------------------------- from an E-step's log-joints (truncated state set)
def expect_from_lpj(logpj, a, cand, H, blocks, soff, moff, table, off=None):
    """E[s] (N, H) under q = softmax(a logpj + off) -- blocks of H one-cause columns from ``soff`` (block c: value blocks[c]),
    table states from ``moff`` (state s: value table[s, j] at latent cand[n, j]; a repeated latent receives both positions);
    every other column carries weight and no value."""
    N = logpj.shape[0]
    q = softmax_rows(a * np.asarray(logpj, dtype=np.float64) + (0.0 if off is None else np.asarray(off)[None, :]))
    es = np.zeros((N, H))
    for c, v in enumerate(blocks):
        es += v * q[:, soff + c * H: soff + (c + 1) * H]
    if table is not None and len(table):
        table = np.asarray(table, dtype=np.float64)
        t = q[:, moff: moff + table.shape[0]] @ table             # (N, Hp)
        for j in range(table.shape[1]):
            np.add.at(es, (np.arange(N), np.asarray(cand)[:, j]), t[:, j])
    return es


def linear_from_lpj(logpj, a, cand, W, blocks, soff, moff, table, mu=None):
    """``expect_from_lpj``, then mu + E[s] W^T."""
    es = expect_from_lpj(logpj, a, cand, W.shape[1], blocks, soff, moff, table)
    return es @ W.T + (0.0 if mu is None else np.asarray(mu)[None, :])


def mca_multi_from_lpj(logpj, lse, cand, state_matrix, Wrho, rho, signed):
    """sum over the S multi-cause columns [1 + H, 1 + H + S) of exp(logpj - lse) Wbar(s), Wbar_d(s) = (sum_{j in s}
    Wrho[c_j, d])^(1/rho) (signed: sign(T) |T|^(1/rho)) from the table of powers ``Wrho`` (H, D) itself: what
    pm_recon_mca_f64 adds to Yhat."""
    logpj, Wrho = np.asarray(logpj, dtype=np.float64), np.asarray(Wrho, dtype=np.float64)
    H = Wrho.shape[0]
    SM = np.asarray(state_matrix) != 0
    out = np.zeros((logpj.shape[0], Wrho.shape[1]))
    for n in range(logpj.shape[0]):
        for s, row in enumerate(SM):
            T = Wrho[np.asarray(cand)[n, row]].sum(axis=0)
            wbar = np.sign(T) * np.abs(T) ** (1. / rho) if signed else T ** (1. / rho)
            out[n] += np.exp(logpj[n, 1 + H + s] - lse[n]) * wbar
    return out


def mca_from_lpj(logpj, cand, state_matrix, W, rho, signed):
    """Columns [null ; H one-cause states ; S multi-cause states over the candidates]: sum_s q_s Wbar(s)."""
    N = logpj.shape[0]
    D, H = W.shape
    q = softmax_rows(np.asarray(logpj, dtype=np.float64))
    out = q[:, 1:1 + H] @ W.T
    mean = mca_mean(W, rho, signed)
    cand = np.asarray(cand)
    cache = {}
    for n in range(N):
        for s, row in enumerate(np.asarray(state_matrix)):
            act = tuple(cand[n, np.nonzero(row)[0]])
            if act not in cache:
                cache[act] = mean(act)
            out[n] += q[n, 1 + H + s] * cache[act]
    return out


def gsc_from_lpj(p, Y, logpj, cand, state_matrix):
    """Columns [null ; H one-cause states ; S multi-cause states over the (sorted) candidates], weights exp(logpj / 2) of
    the doubled-logit pass: sum_s q_s W_s kappa_s(y_n) with kappa from NumPy."""
    N = Y.shape[0]
    H = p["W"].shape[1]
    q = softmax_rows(0.5 * np.asarray(logpj, dtype=np.float64))
    out = np.zeros_like(Y)
    cand = np.asarray(cand)
    for h in range(H):
        out += q[:, 1 + h: 2 + h] * gsc_state_terms(p, Y, [h])[1]
    for n in range(N):
        for s, row in enumerate(np.asarray(state_matrix)):
            act = cand[n, np.nonzero(row)[0]]
            out[n] += q[n, 1 + H + s] * gsc_state_terms(p, Y[n:n + 1], act)[1][0]
    return out


# -------------------------------------------------------------------------------------------------------------- mixtures
def mog_recon(Y, W, pies, sig):
    """sum_h r_nh W_h, r the softmax of log pies_h + log N(y_n; w_h, Sigma_h) (diagonal (H, D) or full (H, D, D))."""
    D, H = W.shape
    Z = np.empty((Y.shape[0], H))
    for h in range(H):
        r = Y - W[:, h][None, :]
        if sig.ndim == 2:
            Z[:, h] = -0.5 * (r * r / sig[h]).sum(1) - 0.5 * np.log(sig[h]).sum()
        else:
            Z[:, h] = -0.5 * (r * np.linalg.solve(sig[h], r.T).T).sum(1) - 0.5 * np.linalg.slogdet(sig[h])[1]
    with np.errstate(divide="ignore"):
        return softmax_rows(Z + np.log(pies)[None, :]) @ W.T


def mop_recon(X, W, pies):
    """sum_h r_nh W_h, r the softmax of log pies_h + sum_d (x log w - w) on the data X the E-step sees."""
    with np.errstate(divide="ignore"):
        Z = X @ np.log(W) - W.sum(0)[None, :] + np.log(pies)[None, :]
    return softmax_rows(Z) @ W.T


def row_rel_err(got, want):
    """max_d |got - want| / max_d |want| per row, the largest over the rows."""
    scale = np.abs(want).max(axis=1)
    return float((np.abs(got - want).max(axis=1) / np.where(scale > 0, scale, 1.0)).max())
