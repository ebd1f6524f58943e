"""NumPy restatement of the masked joints of DESIGN 4.16 (missing values), shared by tests/test_masked_cpu.py and
tests/test_masked_gpu.py: the posterior mean and log sum_s p(s, y_obs) by plain enumeration of every state, the same sums
over a truncated state set rebuilt from a given candidate array, the candidate selections with their scores and the gap at
the selection boundary, and pm_bsc_masked_estep_f64 restated for exact inputs (tests/test_eval_kernels_gpu.py).  An
unobserved value is selected away (np.where), never multiplied.  Not a test module."""
import itertools

import numpy as np
from scipy.special import logsumexp

from recon_reference import mca_mean, softmax_rows


def all_states(H):
    """Every subset of the H latents as a tuple of active indices, the empty set first."""
    return [tuple(np.nonzero(s)[0]) for s in itertools.product([0, 1], repeat=H)]


def truncated_states(H, cand_row, state_matrix):
    """[null ; H singletons ; the table states over this row's candidates]: the columns of the E-step's logpj."""
    cand_row = np.asarray(cand_row)
    return [()] + [(h,) for h in range(H)] + [tuple(cand_row[np.nonzero(r)[0]]) for r in np.asarray(state_matrix)]


def bsc_mean(W, mu=None):
    mu = np.zeros(W.shape[0]) if mu is None else np.asarray(mu, dtype=np.float64)
    return lambda act: mu + W[:, list(act)].sum(axis=1)


def mca_state_mean(W, rho, signed):
    """W_h for a one-cause state (the E-step's energy uses W itself), the rho-combination above, 0 for the null state."""
    comb = mca_mean(W, rho, signed)
    return lambda act: W[:, act[0]].copy() if len(act) == 1 else comb(list(act))


def evaluate(Y, M, states_per_row, mean, H, pi, sigma):
    """(yhat (N, D), log sum_s p(s, y_obs,n) (N,)) with
    log p(s, y_obs) = |s| log pi + (H - |s|) log(1 - pi) - D_n / 2 log(2 pi sigma^2) - sum_d m_d (y_d - ybar_d(s))^2 / (2 sigma^2).
    ``states_per_row``: one list of states (shared by all rows) or a list of N lists."""
    Y = np.asarray(Y, dtype=np.float64)
    M = np.asarray(M) != 0
    N, D = Y.shape
    shared = not (len(states_per_row) == N and isinstance(states_per_row[0], list))
    cache = {}

    def table(states):
        for s in states:
            if s not in cache:
                cache[s] = mean(s)
        means = np.array([cache[s] for s in states])
        sizes = np.array([len(s) for s in states], dtype=np.float64)
        return means, sizes * np.log(pi) + (H - sizes) * np.log(1. - pi)

    yhat, ll = np.empty((N, D)), np.empty(N)
    tab = table(states_per_row) if shared else None
    for n in range(N):
        means, lp = tab if shared else table(states_per_row[n])
        with np.errstate(invalid="ignore"):
            r2 = np.where(M[n][None, :], (np.where(M[n], Y[n], 0.0)[None, :] - means) ** 2, 0.0).sum(axis=1)
        lj = lp - 0.5 * M[n].sum() * np.log(2 * np.pi * sigma ** 2) - 0.5 * r2 / sigma ** 2
        ll[n] = logsumexp(lj) if not np.isnan(lj).any() else np.nan
        yhat[n] = softmax_rows(lj[None, :])[0] @ means
    return yhat, ll


# ------------------------------------------------------------------------------------------------------------ selections
def score_bsc(Y, M, W, mu=None):
    """b_h / sqrt(G_n[h,h]) (0 where G_n[h,h] = 0): the H' LARGEST are selected."""
    M = np.asarray(M) != 0
    X = np.where(M, np.asarray(Y, dtype=np.float64) - (0.0 if mu is None else np.asarray(mu)[None, :]), 0.0)
    b = X @ W
    g = M.astype(np.float64) @ (W * W)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(g > 0, b / np.sqrt(g), 0.0)


def score_mca(Y, M, W):
    """sum_d m_d max(W_dh - y_d, 0): the H' SMALLEST are selected."""
    M = np.asarray(M) != 0
    Yc = np.where(M, Y, 0.0)
    return np.where(M[:, :, None], np.maximum(W[None, :, :] - Yc[:, :, None], 0.0), 0.0).sum(axis=1)


def score_mmca(Y, M, W):
    """MMCA ranks by distance, sum_d m_d (W_dh - y_d)^2: the H' SMALLEST are selected."""
    M = np.asarray(M) != 0
    Yc = np.where(M, Y, 0.0)
    return np.where(M[:, :, None], (W[None, :, :] - Yc[:, :, None]) ** 2, 0.0).sum(axis=1)


def select_bsc(Y, M, W, Hp, mu=None):
    """The H' largest b_h / sqrt(G_n[h,h]) (0 where G_n[h,h] = 0), ascending, ties towards the larger index."""
    return np.argsort(score_bsc(Y, M, W, mu), axis=1, kind="stable")[:, -Hp:]


def select_mca(Y, M, W, Hp):
    """The H' smallest sum_d m_d max(W_dh - y_d, 0), ascending."""
    return np.argsort(score_mca(Y, M, W), axis=1, kind="stable")[:, :Hp]


def select_mmca(Y, M, W, Hp):
    """MMCA ranks by distance: the H' smallest sum_d m_d (W_dh - y_d)^2, ascending."""
    return np.argsort(score_mmca(Y, M, W), axis=1, kind="stable")[:, :Hp]


def boundary_gap(score, Hp, largest):
    """Per row: the relative distance |a - b| / max(|a|, |b|) between the last score selected and the first one left out (the
    H'-th and (H'+1)-th in the ranking's direction); 0 for an exact tie, inf when every latent is selected.  An exact
    comparison of candidate lists against another implementation of the scores means something only where this is well
    above the two implementations' rounding."""
    score = np.asarray(score, dtype=np.float64)
    N, H = score.shape
    if Hp >= H:
        return np.full(N, np.inf)
    srt = np.sort(score, axis=1)
    a, b = (srt[:, H - Hp], srt[:, H - Hp - 1]) if largest else (srt[:, Hp - 1], srt[:, Hp])
    scale = np.maximum(np.abs(a), np.abs(b))
    return np.where(a == b, 0.0, np.abs(a - b) / np.where(scale > 0, scale, 1.0))


def model_scores(kind, params, Y, M):
    """(scores (N, H), True when the largest are selected) of 'bsc', 'mca' or 'mmca'."""
    W = np.asarray(params["W"], dtype=np.float64)
    if kind == "bsc":
        return score_bsc(Y, M, W, params.get("mu")), True
    return (score_mca if kind == "mca" else score_mmca)(Y, M, W), False


# ------------------------------------------------------------- pm_bsc_masked_estep_f64 restated for exact (integer) inputs
def bsc_select_rule(b, g, Hp):
    """The kernel's selection from given b and g: score b / sqrt(g) where g > 0, else 0; a NaN score ranks lowest (as -inf);
    the H' largest, ascending, ties towards the larger index (a stable ascending sort keeps equal scores in index order, so
    the larger index of a tie sits nearer the top)."""
    b, g = np.asarray(b, dtype=np.float64), np.asarray(g, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        score = np.where(g > 0, b / np.sqrt(np.where(g > 0, g, 1.0)), 0.0)
    score = np.where(np.isnan(score), -np.inf, score)
    return np.argsort(score, axis=1, kind="stable")[:, -Hp:]


def bsc_masked_terms(b, g, xnorm2, M, Wt, cand, state_matrix):
    """The two terms of every column of the masked BSC log-joints, [null ; H singletons ; S table states over ``cand``]:
    (|s| (N, K), e (N, K)) with logpj = ppil |s| + ecoef e and
    e_s = |x|^2_obs - 2 sum_{h in s} b_h + sum_{h,h' in s} G_n[h,h'],  G_n[h,h'] = sum_d m_d Wt[h,d] Wt[h',d]
    (the diagonal taken from ``g``).  On integer inputs every sum is exact in f64 in any order."""
    b, g, Wt = (np.asarray(v, dtype=np.float64) for v in (b, g, Wt))
    xnorm2 = np.asarray(xnorm2, dtype=np.float64)
    Mf = (np.asarray(M) != 0).astype(np.float64)
    SM = np.asarray(state_matrix, dtype=np.float64)                    # (S, Hp)
    cand = np.asarray(cand)
    N, H = b.shape
    S = SM.shape[0]
    size = np.concatenate([[0.0], np.ones(H), SM.sum(axis=1)])[None, :].repeat(N, axis=0)
    e = np.empty((N, 1 + H + S))
    e[:, 0] = xnorm2
    e[:, 1:1 + H] = g - 2.0 * b + xnorm2[:, None]
    for n in range(N):
        Wc = Wt[cand[n]]                                               # (Hp, D)
        G = (Wc * Mf[n][None, :]) @ Wc.T
        G[np.diag_indices_from(G)] = g[n, cand[n]]
        e[n, 1 + H:] = xnorm2[n] - 2.0 * (SM @ b[n, cand[n]]) + np.einsum("si,ij,sj->s", SM, G, SM)
    return size, e


# ------------------------------------------------------------------------------------------------------- the four models
def model_terms(kind, params):
    """(mean function, selection function(Y, M, Hp)) of 'bsc', 'mca' or 'mmca' at ``params`` (W (D, H), pi, sigma, mu)."""
    W = np.asarray(params["W"], dtype=np.float64)
    if kind == "bsc":
        mu = params.get("mu")
        return bsc_mean(W, mu), lambda Y, M, Hp: select_bsc(Y, M, W, Hp, mu)
    rho = 21.0 if kind == "mca" else 6.0          # 1 / (1 - 1 / T_rho) at the bound on T: 1.05 for MCA, 1.2 for MMCA
    mean = mca_state_mean(W, rho, kind == "mmca")
    sel = select_mca if kind == "mca" else select_mmca
    return mean, lambda Y, M, Hp: sel(Y, M, W, Hp)


def enumerate_all(kind, params, Y, M):
    H = np.asarray(params["W"]).shape[1]
    mean, _ = model_terms(kind, params)
    return evaluate(Y, M, all_states(H), mean, H, float(params["pi"]), float(params["sigma"]))


def from_candidates(kind, params, Y, M, cand, state_matrix):
    H = np.asarray(params["W"]).shape[1]
    mean, _ = model_terms(kind, params)
    states = [truncated_states(H, c, state_matrix) for c in np.asarray(cand)]
    return evaluate(Y, M, states, mean, H, float(params["pi"]), float(params["sigma"]))
