"""NumPy restatements of encode(), shared by tests/test_encode_cpu.py, tests/test_encode_kernels_gpu.py and
tests/test_encode_gpu.py: mean[n, h] = sum_s q_n(s) s_h and prob[n, h] = sum_s q_n(s) [s_h != 0] from an E-step's (logpj,
candidates, table, blocks) with the union rule for a latent that two candidate positions hold, and the same two marginals by
plain enumeration of every state of the small models.  Not a test module."""
import itertools

import numpy as np

import recon_reference as R


# ---------------------------------------------------------------------- from an E-step's log-joints (truncated state set)
def codes_from_lpj(logpj, a, cand, H, blocks, soff, moff, table, off=None, naive=False):
    """(mean, prob), both (N, H), under q = softmax(a logpj + off).  mean is recon_reference.expect_from_lpj: a latent
    that two positions hold receives both positions' values.  prob: the blocks of non-zero value, plus every table state
    ONCE per latent that any of its positions holds with a non-zero value (the union rule), returned as min(p, 1).
    ``naive``: prob by summing the positions' indicators instead, unclamped -- what the union rule is there to avoid."""
    logpj = np.asarray(logpj, dtype=np.float64)
    N = logpj.shape[0]
    mean = R.expect_from_lpj(logpj, a, cand, H, blocks, soff, moff, table, off=off)
    q = R.softmax_rows(a * logpj + (0.0 if off is None else np.asarray(off)[None, :]))
    prob = np.zeros((N, H))
    for c, v in enumerate(blocks):
        if v != 0:
            prob += q[:, soff + c * H: soff + (c + 1) * H]
    if table is not None and len(table):
        nz = np.asarray(table) != 0                                    # (S, Hp)
        S, Hp = nz.shape
        cand = np.asarray(cand)
        qs = q[:, moff: moff + S]
        for n in range(N):
            if naive:
                act = np.zeros((S, H))
                for j in range(Hp):
                    act[:, cand[n, j]] += nz[:, j]
            else:
                act = np.zeros((S, H), dtype=bool)
                for j in range(Hp):
                    act[:, cand[n, j]] |= nz[:, j]
            prob[n] += qs[n] @ act.astype(np.float64)
    if naive:
        return mean, prob
    with np.errstate(invalid="ignore"):
        return mean, np.where(prob > 1.0, 1.0, prob)                   # (a NaN stays NaN)


# ---------------------------------------------------------------------------------------------------------- enumeration
def _marginals(logjoint, S):
    """(q @ S, q @ [S != 0]) for the (N, states) log-joints and the (states, H) latent values."""
    with np.errstate(invalid="ignore"):
        q = R.softmax_rows(logjoint)
    return q @ S, q @ (S != 0).astype(np.float64)


def enum_linear(Y, W, sigma, values, logp, mu=None):
    """BSC / DSC / TSC: states values^H, log prior sum_h logp[k_h], y ~ N(mu + W s, sigma^2 I)."""
    H = W.shape[1]
    values = np.asarray(values, dtype=np.float64)
    idx = np.array(list(itertools.product(range(len(values)), repeat=H)))
    S = values[idx]
    with np.errstate(invalid="ignore"):
        lp = np.asarray(logp, dtype=np.float64)[idx].sum(axis=1)
    keep = np.isfinite(lp)                       # a state of zero prior contributes nothing
    S, lp = S[keep], lp[keep]
    means = S @ W.T + (0.0 if mu is None else np.asarray(mu)[None, :])
    r2 = ((Y[:, None, :] - means[None, :, :]) ** 2).sum(-1)
    return _marginals(lp[None, :] - 0.5 * r2 / sigma ** 2, S)


def enum_mca(Y, W, rho, signed, pi, sigma):
    H = W.shape[1]
    S = R.enum_states([0, 1], H)
    mean = R.mca_mean(W, rho, signed)
    means = np.array([mean(np.nonzero(s)[0]) for s in S])
    lp = S.sum(1) * np.log(pi) + (H - S.sum(1)) * np.log(1 - pi)
    r2 = ((Y[:, None, :] - means[None, :, :]) ** 2).sum(-1)
    return _marginals(lp[None, :] - 0.5 * r2 / sigma ** 2, S)


def gsc_support_terms(p, Y, active):
    """(log p(s, y_n) up to a constant common to all supports (N,), kappa_s(y_n) = E[z_s | s, y_n] scattered into (N, H))."""
    W, mu, Psi = p["W"], np.asarray(p["mu"], dtype=np.float64), p["psi_sq"]
    D, H = W.shape
    pi = np.broadcast_to(np.asarray(p["pi"], dtype=np.float64), (H,))
    Sig = R._gsc_sigma(p, D)
    a = np.asarray(active, dtype=int)
    Wa, Pa = W[:, a], Psi[np.ix_(a, a)]
    C = Sig + Wa @ Pa @ Wa.T
    r = Y - (Wa @ mu[a])[None, :]
    Cr = np.linalg.solve(C, r.T)
    logp = np.log(pi[a]).sum() + np.log(1 - np.delete(pi, a)).sum() - 0.5 * np.linalg.slogdet(C)[1] \
        - 0.5 * (r * Cr.T).sum(axis=1)
    kap = np.zeros((Y.shape[0], H))
    kap[:, a] = mu[a][None, :] + (Pa @ Wa.T @ Cr).T
    return logp, kap


def enum_gsc(p, Y):
    """GSC: mean = E[s_h z_h | y_n] = sum_s q_n(s) kappa_s(y_n)_h, prob = E[s_h | y_n], over all 2^H supports."""
    H = p["W"].shape[1]
    sets = [np.nonzero(s)[0] for s in itertools.product([0, 1], repeat=H)]
    terms = [gsc_support_terms(p, Y, a) for a in sets]
    q = R.softmax_rows(np.stack([t[0] for t in terms], axis=1))
    ind = np.array([[1.0 if h in a else 0.0 for h in range(H)] for a in sets])
    return sum(q[:, k:k + 1] * terms[k][1] for k in range(len(sets))), q @ ind


def gsc_from_lpj(p, Y, logpj, cand, state_matrix):
    """Columns [null ; H one-cause states ; S multi-cause states over the (sorted) candidates], weights exp(logpj / 2) of
    the doubled-logit pass: (sum_s q_s kappa_s(y_n), sum_s q_s [h in s]) with kappa from NumPy."""
    N = Y.shape[0]
    H = p["W"].shape[1]
    q = R.softmax_rows(0.5 * np.asarray(logpj, dtype=np.float64))
    mean, prob = np.zeros((N, H)), np.zeros((N, H))
    cand = np.asarray(cand)
    for h in range(H):
        mean += q[:, 1 + h: 2 + h] * gsc_support_terms(p, Y, [h])[1]
        prob[:, h] += q[:, 1 + h]
    for n in range(N):
        for s, row in enumerate(np.asarray(state_matrix)):
            act = cand[n, np.nonzero(row)[0]]
            mean[n] += q[n, 1 + H + s] * gsc_support_terms(p, Y[n:n + 1], act)[1][0]
            prob[n, act] += q[n, 1 + H + s]
    return mean, prob


def mixture_resp(kind, X, W, pies, sig=None):
    """Responsibilities (N, H) of MoG (diagonal or full ``sig``) / MoP on the data ``X`` the E-step sees."""
    H = W.shape[1]
    with np.errstate(divide="ignore"):
        if kind.startswith("mop"):
            return R.softmax_rows(X @ np.log(W) - W.sum(0)[None, :] + np.log(pies)[None, :])
        Z = np.empty((X.shape[0], H))
        for h in range(H):
            r = X - W[:, h][None, :]
            if sig.ndim == 2:
                Z[:, h] = -0.5 * (r * r / sig[h]).sum(1) - 0.5 * np.log(sig[h]).sum()
            else:
                Z[:, h] = -0.5 * (r * np.linalg.solve(sig[h], r.T).T).sum(1) - 0.5 * np.linalg.slogdet(sig[h])[1]
        return R.softmax_rows(Z + np.log(pies)[None, :])


def rel_err(got, want):
    """max |got - want| relative to the largest entry of ``want`` (at least 1e-300)."""
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))
