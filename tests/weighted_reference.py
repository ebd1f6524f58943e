"""NumPy restatement of the weighted joints of DESIGN 4.22 (per-entry noise weights), shared by tests/test_weighted_cpu.py
and the weighted GPU tests: entry (n, d) is observed with noise variance sigma^2 / omega_nd, omega_nd = 0 = not observed, and

    log p(s, y_n | omega_n) = log p(s) - sum_d omega_nd (x_nd - ybar_d(s))^2 / (2 sigma^2) - D_n / 2 log(2 pi sigma^2)
                              + 1/2 sum_{d: omega_nd > 0} log omega_nd,      D_n = #{d: omega_nd > 0}

in the direct form for every model (MCA / MMCA: sum omega (y - Wbar)^2 with the rho-combination Wbar).  Per-row log-joints,
log-likelihood, posterior mean and variance by plain enumeration of a state list -- every state, or the truncated set rebuilt
from a candidate array ([null ; H singletons ; table states], masked_reference.truncated_states) -- and the candidate
selections with their scores.  A value at weight 0 is selected away (np.where), never multiplied.  Not a test module."""
import numpy as np
from scipy.special import logsumexp

import masked_reference as MR
from recon_reference import softmax_rows

all_states = MR.all_states
truncated_states = MR.truncated_states
boundary_gap = MR.boundary_gap


def log_joints(y, om, means, sizes, H, pi, sigma):
    """The (K,) log-joints of one row against the (K, D) state means (x = y for MCA, y with mu inside ``means`` for BSC)."""
    on = om > 0
    with np.errstate(invalid="ignore", over="ignore"):
        r2 = np.where(on[None, :], om[None, :] * (np.where(on, y, 0.0)[None, :] - means) ** 2, 0.0).sum(axis=1)
    return (sizes * np.log(pi) + (H - sizes) * np.log(1. - pi) - 0.5 * on.sum() * np.log(2 * np.pi * sigma ** 2)
            + 0.5 * np.log(om[on]).sum() - 0.5 * r2 / sigma ** 2)


def evaluate(Y, Om, states_per_row, mean, H, pi, sigma):
    """(yhat (N, D), log sum_s p(s, y_n | omega_n) (N,), V (N, D)): posterior mean and variance of the noiseless value
    ybar(s) and the log-likelihood rows.  ``states_per_row``: one list of states (shared by all rows) or a list of N lists."""
    Y = np.asarray(Y, dtype=np.float64)
    Om = np.asarray(Om, dtype=np.float64)
    N, D = Y.shape
    shared = not (len(states_per_row) == N and isinstance(states_per_row[0], list))
    cache = {}

    def table(states):
        for s in states:
            if s not in cache:
                cache[s] = mean(s)
        return np.array([cache[s] for s in states]), np.array([len(s) for s in states], dtype=np.float64)

    yhat, ll, var = np.empty((N, D)), np.empty(N), np.empty((N, D))
    tab = table(states_per_row) if shared else None
    for n in range(N):
        means, sizes = tab if shared else table(states_per_row[n])
        lj = log_joints(Y[n], Om[n], means, sizes, H, pi, sigma)
        ll[n] = logsumexp(lj) if not np.isnan(lj).any() else np.nan
        q = softmax_rows(lj[None, :])[0]
        yhat[n] = q @ means
        var[n] = q @ (means - yhat[n][None, :]) ** 2
    return yhat, ll, var


# ------------------------------------------------------------------------------------------------------------ selections
def score_bsc(Y, Om, W, mu=None):
    """b_h / sqrt(G_n[h,h]) with b = W^T diag(omega) x, G_n = W^T diag(omega) W (0 where G_n[h,h] = 0): the H' LARGEST."""
    Om = np.asarray(Om, dtype=np.float64)
    on = Om > 0
    X = np.where(on, np.asarray(Y, dtype=np.float64) - (0.0 if mu is None else np.asarray(mu)[None, :]), 0.0)
    b = (Om * X) @ W
    g = Om @ (W * W)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(g > 0, b / np.sqrt(np.where(g > 0, g, 1.0)), 0.0)


def score_mca(Y, Om, W):
    """sum_d omega_d max(W_dh - y_d, 0): the H' SMALLEST are selected."""
    Om = np.asarray(Om, dtype=np.float64)
    on = Om > 0
    Yc = np.where(on, Y, 0.0)
    return np.where(on[:, :, None], Om[:, :, None] * np.maximum(W[None, :, :] - Yc[:, :, None], 0.0), 0.0).sum(axis=1)


def score_mmca(Y, Om, W):
    """sum_d omega_d (W_dh - y_d)^2: the H' SMALLEST are selected."""
    Om = np.asarray(Om, dtype=np.float64)
    on = Om > 0
    Yc = np.where(on, Y, 0.0)
    return np.where(on[:, :, None], Om[:, :, None] * (W[None, :, :] - Yc[:, :, None]) ** 2, 0.0).sum(axis=1)


def model_scores(kind, params, Y, Om):
    """(scores (N, H), True when the largest are selected) of 'bsc', 'mca' or 'mmca'."""
    W = np.asarray(params["W"], dtype=np.float64)
    if kind == "bsc":
        return score_bsc(Y, Om, W, params.get("mu")), True
    return (score_mca if kind == "mca" else score_mmca)(Y, Om, W), False


def select(kind, params, Y, Om, Hp):
    """The candidates (N, H'), ascending: the H' largest BSC scores (ties towards the larger index: a stable ascending sort
    keeps equal scores in index order; a row of zero weights gets the H' largest indices), the H' smallest MCA / MMCA ones."""
    sc, largest = model_scores(kind, params, Y, Om)
    order = np.argsort(sc, axis=1, kind="stable")
    return order[:, -Hp:] if largest else order[:, :Hp]


# ------------------------------------------------------------------------------------------------------- the three models
def model_mean(kind, params):
    """ybar(s) of 'bsc' (mu + sum of the active columns), 'mca' (rho = 21) or 'mmca' (rho = 6, signed)."""
    W = np.asarray(params["W"], dtype=np.float64)
    if kind == "bsc":
        return MR.bsc_mean(W, params.get("mu"))
    return MR.mca_state_mean(W, 21.0 if kind == "mca" else 6.0, kind == "mmca")


def enumerate_all(kind, params, Y, Om):
    H = np.asarray(params["W"]).shape[1]
    return evaluate(Y, Om, all_states(H), model_mean(kind, params), H, float(params["pi"]), float(params["sigma"]))


def from_candidates(kind, params, Y, Om, cand, state_matrix):
    H = np.asarray(params["W"]).shape[1]
    states = [truncated_states(H, c, state_matrix) for c in np.asarray(cand)]
    return evaluate(Y, Om, states, model_mean(kind, params), H, float(params["pi"]), float(params["sigma"]))


def joints_from_candidates(kind, params, Y, Om, cand, state_matrix):
    """(lp (N, K), means (N, K, D)): the rows' log-joints in the column order of the E-step's logpj over the truncated sets
    rebuilt from ``cand``, and the states' means ybar(s) in the same order."""
    Y, Om = np.asarray(Y, dtype=np.float64), np.asarray(Om, dtype=np.float64)
    H = np.asarray(params["W"]).shape[1]
    mean = model_mean(kind, params)
    lp, mm = [], []
    for n, c in enumerate(np.asarray(cand)):
        states = truncated_states(H, c, state_matrix)
        means = np.array([mean(s) for s in states])
        sizes = np.array([len(s) for s in states], dtype=np.float64)
        lp.append(log_joints(Y[n], Om[n], means, sizes, H, float(params["pi"]), float(params["sigma"])))
        mm.append(means)
    return np.array(lp), np.array(mm)
