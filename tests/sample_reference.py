"""NumPy restatement of sample_posterior(), shared by tests/test_sample_cpu.py, tests/test_sample_gpu.py and
tests/test_sample_abi_gpu.py: the categorical draw from a row of log-joints by ``np.cumsum``, the active list of a drawn
column, and the per-state means ybar(s) -- plain loops.  The column layout is pm_recon_expect_f64's
(tests/recon_reference.py).  Not a test module."""
import numpy as np
from scipy.special import logsumexp

import recon_reference as R

U_MAX = np.nextafter(1.0, 0.0)


def weights(lp, a=1.0, off=None, floor=0.0, null_col=-1, lse=None):
    """w (N, K) = exp(a lp + off - lse), lse the rows' log-sum-exp unless given (GSC: zeros, the E-step's un-normalised
    weights), raised to ``floor`` in every column but ``null_col``; NaN rows stay NaN."""
    Z = a * np.asarray(lp, dtype=np.float64) + (0.0 if off is None else np.asarray(off)[None, :])
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.exp(Z - (logsumexp(Z, axis=1, keepdims=True) if lse is None else np.asarray(lse).reshape(-1, 1)))
    if floor > 0.0:
        keep = np.ones(w.shape[1], dtype=bool)
        if null_col >= 0:
            keep[null_col] = False
        w[:, keep] = np.where(np.isnan(w[:, keep]), np.nan, np.maximum(w[:, keep], floor))
    return w


def cdfs(lp, **kw):
    """(N, K) running sums of the weights in ascending column order (``np.cumsum``)."""
    return np.cumsum(weights(lp, **kw), axis=1)


def draw_states(lp, U, **kw):
    """idx (N, M): the smallest k with u c_{K-1} < c_k; u clamped into [0, nextafter(1, 0)] (NaN -> 0); -1 for a row whose
    weights hold a NaN or do not sum to a positive finite value."""
    c = cdfs(lp, **kw)
    U = np.asarray(U, dtype=np.float64)
    N, M = U.shape
    idx = np.full((N, M), -1, dtype=np.int32)
    for n in range(N):
        C = c[n, -1]
        if np.isnan(c[n]).any() or not (C > 0.0) or not np.isfinite(C):
            continue
        with np.errstate(invalid="ignore"):
            u = np.where(U[n] >= 0.0, U[n], 0.0)
        u = np.where(u < 1.0, u, U_MAX)
        idx[n] = np.searchsorted(c[n], u * C, side="right")
    return idx


def nudge(U, c, rel=1e-9):
    """Every u within ``rel`` c_{K-1} of a CDF edge of the reference moved to the middle of its interval (the interval of
    the column the reference draws): no draw is left out, and the summation order of the CDF cannot decide one."""
    U = np.array(U, dtype=np.float64, copy=True)
    moved = 0
    for n in range(U.shape[0]):
        C = c[n, -1]
        if not (C > 0.0) or np.isnan(c[n]).any():
            continue
        edges = np.concatenate([[0.0], c[n]])
        near = np.abs(edges[None, :] - (U[n] * C)[:, None]).min(axis=1) <= rel * C
        for m in np.nonzero(near)[0]:
            k = min(int(np.searchsorted(c[n], U[n, m] * C, side="right")), len(c[n]) - 1)
            while k < len(c[n]) - 1 and edges[k + 1] - edges[k] <= 4 * rel * C:           # (a sliver: take the next wide one)
                k += 1
            U[n, m] = 0.5 * (edges[k] + edges[k + 1]) / C
            moved += 1
    return U, moved


def active_list(idx, cand, H, blocks, soff, moff, table, A):
    """(act_idx (N, M, A) int32, act_val (N, M, A)): entries in ascending candidate position, unused slots (-1, 0), a draw
    of -1 (-1, NaN) in every slot."""
    N, M = idx.shape
    ai = np.full((N, M, A), -1, dtype=np.int32)
    av = np.zeros((N, M, A))
    S = 0 if table is None else len(table)
    for n in range(N):
        for m in range(M):
            k = idx[n, m]
            if k < 0:
                av[n, m] = np.nan
                continue
            j = 0
            if soff <= k < soff + len(blocks) * H:
                c = (k - soff) // H
                ai[n, m, 0], av[n, m, 0] = (k - soff) - c * H, blocks[c]
            elif S and moff <= k < moff + S:
                for pos, v in enumerate(np.asarray(table)[k - moff]):
                    if v != 0 and j < A:
                        ai[n, m, j], av[n, m, j] = cand[n, pos], v
                        j += 1
    return ai, av


def latents_from_active(ai, av, H):
    """S (M, N, H): the list scattered (a latent listed twice receives both values); NaN rows for a draw of -1."""
    N, M, A = ai.shape
    S = np.zeros((M, N, H))
    for n in range(N):
        for m in range(M):
            if np.isnan(av[n, m]).any():
                S[m, n] = np.nan
                continue
            for j in range(A):
                if ai[n, m, j] >= 0:
                    S[m, n, ai[n, m, j]] += av[n, m, j]
    return S


def decode_linear(ai, av, W, mu=None):
    """Ys (M, N, D) = mu + sum_j act_val_j W[:, act_idx_j], one term after the other in ascending j."""
    N, M, A = ai.shape
    D = W.shape[0]
    Ys = np.empty((M, N, D))
    for n in range(N):
        for m in range(M):
            acc = np.zeros(D) if mu is None else np.array(mu, dtype=np.float64).reshape(-1).copy()
            if np.isnan(av[n, m]).any():
                acc[:] = np.nan
            for j in range(A):
                if ai[n, m, j] >= 0:
                    acc = acc + av[n, m, j] * W[:, ai[n, m, j]]
            Ys[m, n] = acc
    return Ys


def decode_mca(idx, cand, state_matrix, W, rho, signed):
    """Ys (M, N, D): 0 for the null column, W_h for a one-cause column, the rho-combination over the state's candidates for a
    multi-cause column (recon_reference.mca_mean), NaN for a draw of -1."""
    N, M = idx.shape
    D, H = W.shape
    mean = R.mca_mean(W, rho, signed)
    SM = np.asarray(state_matrix)
    Ys = np.empty((M, N, D))
    for n in range(N):
        for m in range(M):
            k = idx[n, m]
            if k < 0:
                Ys[m, n] = np.nan
            elif k == 0:
                Ys[m, n] = 0.0
            elif k <= H:
                Ys[m, n] = W[:, k - 1]
            else:
                Ys[m, n] = mean(np.asarray(cand)[n, np.nonzero(SM[k - 1 - H])[0]])
    return Ys


def state_means_linear(n, cand, W, H, K, blocks, soff, moff, table, mu=None):
    """ybar(s) (K, D) of every column of row n: what reconstruct averages for the linear models."""
    idx = np.arange(K, dtype=np.int32)[None, :]
    A = max(1, 0 if table is None else int((np.asarray(table) != 0).sum(axis=1).max()))
    ai, av = active_list(idx, np.asarray(cand)[n:n + 1], H, blocks, soff, moff, table, A)
    return decode_linear(ai, av, W, mu)[:, 0, :]


GSC_WEIGHTS = dict(a=0.5, floor=np.finfo(np.float64).tiny, null_col=0)      # + lse = zeros(N): pm_recon_gsc_moments2_f64's


def gsc_posterior(p, y, active):
    """(kappa, Lambda^-1) of z | s, y for the support ``active`` (in the order given): Lambda = W_a^T Sigma^-1 W_a + (Psi_aa)^-1,
    kappa = mu_a + Lambda^-1 W_a^T Sigma^-1 (y - W_a mu_a)."""
    a = np.asarray(active, dtype=int)
    W, mu, Psi = np.asarray(p["W"]), np.asarray(p["mu"], dtype=np.float64), np.asarray(p["psi_sq"])
    Sinv = np.linalg.inv(R._gsc_sigma(p, W.shape[0]))
    Wa = W[:, a]
    Lam = Wa.T @ Sinv @ Wa + np.linalg.inv(Psi[np.ix_(a, a)])
    cov = np.linalg.inv(Lam)
    cov = 0.5 * (cov + cov.T)
    return mu[a] + cov @ (Wa.T @ Sinv @ (y - Wa @ mu[a])), cov


def gsc_draw(p, y, active, eps):
    """z = kappa + L eps[:g], L the lower Cholesky factor of Lambda^-1 with the positions in the order of ``active``."""
    kappa, cov = gsc_posterior(p, y, active)
    return kappa + np.linalg.cholesky(cov) @ np.asarray(eps)[:len(kappa)]


def gsc_active_list(idx, cand, state_matrix, p, Y, E, A):
    """The list format of ``active_list`` with the values z of each draw: columns [null ; H singletons ; S multi-cause states
    over the candidates in ascending position]."""
    N, M = idx.shape
    H = np.asarray(p["W"]).shape[1]
    SM = np.asarray(state_matrix)
    ai = np.full((N, M, A), -1, dtype=np.int32)
    av = np.zeros((N, M, A))
    for n in range(N):
        for m in range(M):
            k = idx[n, m]
            if k < 0:
                av[n, m] = np.nan
            elif k >= 1:
                act = [k - 1] if k <= H else list(np.asarray(cand)[n, np.nonzero(SM[k - 1 - H])[0]])
                ai[n, m, :len(act)] = act
                av[n, m, :len(act)] = gsc_draw(p, Y[n], act, E[n, m])
    return ai, av


def stratified(M):
    return (np.arange(M) + 0.5) / M
