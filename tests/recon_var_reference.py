"""NumPy restatements of reconstruct(variance=True) on top of tests/recon_reference.py, shared by
tests/test_reconstruct_var_cpu.py, tests/test_reconstruct_var_gpu.py and tests/test_reconstruct_var_abi_gpu.py: the posterior
variance of the noiseless value in the centred form sum_s q (ybar(s) - yhat)^2 (+ the spread of z | s, y for GSC) by plain
enumeration of every state, the same sum over a truncated state set rebuilt from an E-step's (logpj, candidates), and the
second moments m2 / p the kernels form from a log-joint row.  Every function returns ``Moments(yhat, V, E2)``: the posterior mean,
the CENTRED variance and the second moment E[ybar^2] (the scale of the tolerance; E2 - yhat^2 is the moment form of V).  Not a
test module."""
import collections
import itertools

import numpy as np

import recon_reference as R

Moments = collections.namedtuple("Moments", "yhat V E2")

# per row: max_d |V - V_ref| <= VTOL max_d E_ref[ybar_d^2] (2e-11 from yhat^2 at the project's row-relative 1e-11
# on yhat, 1e-11 from the second moment through the same expectation and product, the rest margin)
VTOL = 4e-11


def from_states(q, means, extra=None):
    """q (N, S) weights, means (S, D) or (N, S, D) the states' ybar, extra (S, D) or (N, S, D) a variance inside the state
    (GSC: diag W_s Lambda_s^-1 W_s^T)."""
    means = np.asarray(means, dtype=np.float64)
    if means.ndim == 2:
        means = np.broadcast_to(means[None], (q.shape[0],) + means.shape)
    with np.errstate(invalid="ignore"):
        yhat = np.einsum("ns,nsd->nd", q, means)
        V = np.einsum("ns,nsd->nd", q, (means - yhat[:, None, :]) ** 2)
        E2 = np.einsum("ns,nsd->nd", q, means ** 2)
        if extra is not None:
            extra = np.asarray(extra, dtype=np.float64)
            if extra.ndim == 2:
                extra = np.broadcast_to(extra[None], means.shape)
            e = np.einsum("ns,nsd->nd", q, extra)
            V, E2 = V + e, E2 + e
    return Moments(yhat, V, E2)


def row_err(got, ref):
    """max_d |got - V_ref| / max_d E_ref[ybar_d^2] per row, the largest over the rows."""
    scale = np.abs(ref.E2).max(axis=1)
    return float((np.abs(got - ref.V).max(axis=1) / np.where(scale > 0, scale, 1.0)).max())


# ---------------------------------------------------------------------------------------------------------- enumeration
def _gauss_q(Y, means, log_prior, var):
    r2 = ((Y[:, None, :] - means[None, :, :]) ** 2).sum(-1)
    with np.errstate(invalid="ignore"):
        return R.softmax_rows(log_prior[None, :] - 0.5 * r2 / var)


def enum_linear(Y, W, sigma, values, logp, mu=None):
    """BSC / DSC / TSC: states values^H, log prior sum_h logp[k_h], mean mu + W s."""
    H = W.shape[1]
    values = np.asarray(values, dtype=np.float64)
    idx = np.array(list(itertools.product(range(len(values)), repeat=H)))
    with np.errstate(invalid="ignore"):
        lp = np.asarray(logp, dtype=np.float64)[idx].sum(axis=1)
    keep = np.isfinite(lp)
    means = values[idx][keep] @ W.T + (0.0 if mu is None else np.asarray(mu)[None, :])
    return from_states(_gauss_q(Y, means, lp[keep], sigma ** 2), means)


def enum_mca(Y, W, rho, signed, pi, sigma):
    H = W.shape[1]
    S = R.enum_states([0, 1], H)
    mean = R.mca_mean(W, rho, signed)
    means = np.array([mean(np.nonzero(s)[0]) for s in S])
    lp = S.sum(1) * np.log(pi) + (H - S.sum(1)) * np.log(1 - pi)
    return from_states(_gauss_q(Y, means, lp, sigma ** 2), means)


def gsc_state_cov(p, active):
    """diag(W_s Lambda_s^-1 W_s^T) (D,) of the support ``active``: Lambda_s^-1 = Psi_s - Psi_s W_s^T C_s^-1 W_s Psi_s, the
    covariance of z_s given s and y (it does not depend on y), beside ``recon_reference.gsc_state_terms``."""
    W, Psi = p["W"], p["psi_sq"]
    D = W.shape[0]
    a = np.asarray(active, dtype=int)
    if not a.size:
        return np.zeros(D)
    Wa, Pa = W[:, a], Psi[np.ix_(a, a)]
    C = R._gsc_sigma(p, D) + Wa @ Pa @ Wa.T
    Li = Pa - Pa @ Wa.T @ np.linalg.solve(C, Wa @ Pa)
    return np.einsum("da,ab,db->d", Wa, Li, Wa)


def gsc_from_sets(p, Y, sets_per_row, a=None, logpj_rows=None):
    """Over each row's own list of supports (rows that share the list object are evaluated together), weights from NumPy's
    densities -- or, with ``logpj_rows`` (one array of log-joints per row, in the order of its list), softmax(a logpj)."""
    N, D = Y.shape
    out = [np.empty((N, D)) for _ in range(3)]
    groups = {}
    for n, sets in enumerate(sets_per_row):
        groups.setdefault(id(sets), (sets, []))[1].append(n)
    for sets, rows in groups.values():
        rows = np.array(rows)
        terms = [R.gsc_state_terms(p, Y[rows], s) for s in sets]
        if logpj_rows is None:
            q = R.softmax_rows(np.stack([t[0] for t in terms], axis=1))
        else:
            q = R.softmax_rows(a * np.stack([logpj_rows[n] for n in rows]))
        means = np.stack([t[1] for t in terms], axis=1)
        extra = np.stack([gsc_state_cov(p, s) for s in sets])
        for o, v in zip(out, from_states(q, means, extra)):
            o[rows] = v
    return Moments(*out)


def enum_gsc(p, Y):
    H = p["W"].shape[1]
    sets = [np.nonzero(s)[0] for s in itertools.product([0, 1], repeat=H)]
    return gsc_from_sets(p, Y, [sets] * len(Y))


def _mix(r, W):
    return from_states(r, np.ascontiguousarray(W.T))


def mog(Y, W, pies, sig):
    D, H = W.shape
    Z = np.empty((Y.shape[0], H))
    for h in range(H):
        r = Y - W[:, h][None, :]
        if sig.ndim == 2:
            Z[:, h] = -0.5 * (r * r / sig[h]).sum(1) - 0.5 * np.log(sig[h]).sum()
        else:
            Z[:, h] = -0.5 * (r * np.linalg.solve(sig[h], r.T).T).sum(1) - 0.5 * np.linalg.slogdet(sig[h])[1]
    with np.errstate(divide="ignore"):
        return _mix(R.softmax_rows(Z + np.log(pies)[None, :]), W)


def mop(X, W, pies):
    with np.errstate(divide="ignore"):
        Z = X @ np.log(W) - W.sum(0)[None, :] + np.log(pies)[None, :]
    return _mix(R.softmax_rows(Z), W)


# ---------------------------------------------------------------------- from an E-step's log-joints (truncated state set)
def linear_from_lpj(logpj, a, cand, W, blocks, soff, moff, table, mu=None, off=None):
    """Columns as ``recon_reference.expect_from_lpj``: every column is a state with its own mean -- a one-cause column of
    block c the mean blocks[c] W_h, a table column sum_j table[s, j] W_{cand[n, j]} (a repeated latent counted at both
    positions), every other column 0 -- plus mu."""
    logpj = np.asarray(logpj, dtype=np.float64)
    N, K = logpj.shape
    D, H = W.shape
    q = R.softmax_rows(a * logpj + (0.0 if off is None else np.asarray(off)[None, :]))
    M = np.zeros((N, K, D))
    for c, v in enumerate(blocks):
        M[:, soff + c * H: soff + (c + 1) * H, :] = (v * W.T)[None]
    if table is not None and len(table):
        table = np.asarray(table, dtype=np.float64)
        Wc = W[:, np.asarray(cand)]                                       # (D, N, Hp)
        M[:, moff: moff + table.shape[0], :] = np.einsum("sp,dnp->nsd", table, Wc)
    if mu is not None:
        M = M + np.asarray(mu)[None, None, :]
    return from_states(q, M)


def mca_from_lpj(logpj, cand, state_matrix, W, rho, signed):
    """Columns [null ; H one-cause states ; S multi-cause states over the candidates]."""
    logpj = np.asarray(logpj, dtype=np.float64)
    N, K = logpj.shape
    D, H = W.shape
    q = R.softmax_rows(logpj)
    M = np.zeros((N, K, D))
    M[:, 1:1 + H, :] = W.T[None]
    mean = R.mca_mean(W, rho, signed)
    cand = np.asarray(cand)
    cache = {}
    for n in range(N):
        for s, row in enumerate(np.asarray(state_matrix)):
            act = tuple(cand[n, np.nonzero(row)[0]])
            if act not in cache:
                cache[act] = mean(act)
            M[n, 1 + H + s] = cache[act]
    return from_states(q, M)


def gsc_from_lpj(p, Y, logpj, cand, state_matrix):
    """Columns [null ; H one-cause states ; S multi-cause states over the (sorted) candidates], weights exp(logpj / 2) of the
    doubled-logit pass; kappa and Lambda^-1 from NumPy."""
    H = p["W"].shape[1]
    cand, logpj = np.asarray(cand), np.asarray(logpj, dtype=np.float64)
    singles = [np.array([], dtype=int)] + [np.array([h]) for h in range(H)]
    cache, sets = {}, []
    for n in range(len(Y)):
        key = tuple(cand[n])
        if key not in cache:
            cache[key] = singles + [cand[n, np.nonzero(row)[0]] for row in np.asarray(state_matrix)]
        sets.append(cache[key])
    return gsc_from_sets(p, Y, sets, a=0.5, logpj_rows=logpj)


# ------------------------------------------------------------------------------------------- what the kernels form
def moments2_from_lpj(logpj, a, cand, H, blocks, soff, moff, table, off=None):
    """(m2 (N, H), p (N, Hp (Hp - 1) / 2)) of pm_recon_moments2_f64: m2 the second moment per latent (a repeated latent receives
    both positions), p_ij = sum_s q v_i v_j over the table states, pairs of positions in the order (0,1), (0,2), ..."""
    logpj = np.asarray(logpj, dtype=np.float64)
    N = logpj.shape[0]
    q = R.softmax_rows(a * logpj + (0.0 if off is None else np.asarray(off)[None, :]))
    m2 = np.zeros((N, H))
    for c, v in enumerate(blocks):
        m2 += v * v * q[:, soff + c * H: soff + (c + 1) * H]
    if table is None or not len(table):
        return m2, np.zeros((N, 0))
    table = np.asarray(table, dtype=np.float64)
    Hp = table.shape[1]
    qt = q[:, moff: moff + table.shape[0]]
    t2 = qt @ (table * table)
    for j in range(Hp):
        np.add.at(m2, (np.arange(N), np.asarray(cand)[:, j]), t2[:, j])
    pairs = [(i, j) for i in range(Hp) for j in range(i + 1, Hp)]
    p = np.stack([qt @ (table[:, i] * table[:, j]) for i, j in pairs], axis=1) if pairs else np.zeros((N, 0))
    return m2, p


def finish(m2, p, cand, W, yhat, mu=None, V0=None):
    """V of pm_gemm_nt_rows_f64 against W o W (or ``V0``, what pm_recon_var_finish_f64 is handed) + pm_recon_var_finish_f64:
    the moment form, clamped at 0."""
    V = m2 @ (W * W).T if V0 is None else np.array(V0, dtype=np.float64)
    if p is not None and p.shape[1]:
        Hp = np.asarray(cand).shape[1]
        Wc = W[:, np.asarray(cand)]                                       # (D, N, Hp)
        k = 0
        for i in range(Hp):
            for j in range(i + 1, Hp):
                V = V + 2.0 * p[:, k:k + 1] * (Wc[:, :, i] * Wc[:, :, j]).T
                k += 1
    c = yhat - (0.0 if mu is None else np.asarray(mu)[None, :])
    V = V - c * c
    with np.errstate(invalid="ignore"):
        return np.where(V < 0, 0.0, V)


def calibration(yhat, V, clean):
    """sum (yhat - ybar_clean)^2 / sum V: 1 in expectation when V is the posterior variance of the model the data came from."""
    return float(((yhat - clean) ** 2).sum() / V.sum())
