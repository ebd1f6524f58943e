"""Plain longdouble restatements of the exact-enumeration entries (include/prosper_hip.h: pm_loglik_exact_*, pm_recon_exact_*;
DESIGN 4.13, 4.18) on the KERNELS' operands -- P, G, logp, values; Wrho, lp1, lp0; P, M, Psi, mu, logp -- and not on model
parameters, so that a test can hand in operands no model produces.  NumPy with np.longdouble, no torch.  Shared by
tests/test_exact_kernels_cpu.py (which pins every function here three ways) and tests/test_exact_kernels_gpu.py.  Not a test
module.

  lin_rows / lin_means, mca_rows / mca_means, gsc_rows / gsc_means: by enumerating every state, in the state order and with
      the algebra the header states (GSC: a hand-written Cholesky per support, determinant lemma and Woodbury).
  lin_block_rows / lin_block_means, mca_disjoint_rows / mca_disjoint_means, gsc_block_rows / gsc_block_means: closed forms
      for operands that factorise (block-diagonal G; every dimension owned by one cause; block-diagonal M and Psi): a sum over
      blocks of small enumerations, usable at any H.
  total_fixed_order: ex_total_kernel's order of additions, in float64: the bits of total[0] given the returned rows.
  loglik_plan / recon_plan: pm_loglik_exact_plan and pm_recon_exact_plan restated from the header's prose.
"""
import numpy as np

LD = np.longdouble
PM_OK, PM_EINVAL, PM_ERANGE = 0, -1, -2
LIN, MCA, GSC = 0, 1, 2
PLAN_LEN = 10


def _ld(a):
    return np.asarray(a, dtype=LD)


def lse_rows(Z):
    """log sum_s exp Z[n, s] and the weights exp(Z - lse): an all -inf row gives (-inf, 0), a NaN entry a NaN row."""
    Z = _ld(Z)
    with np.errstate(invalid="ignore", over="ignore"):
        m = Z.max(axis=1, keepdims=True)
        safe = np.where(np.isfinite(m), m, LD(0))
        e = np.exp(Z - safe)
        s = e.sum(axis=1, keepdims=True)
        v = np.where(np.isnan(s), LD("nan"), np.where(m == -np.inf, -LD("inf"), safe + np.log(np.where(s > 0, s, LD(1)))))
        q = e / np.where(s > 0, s, LD(1))
    return v[:, 0], q


# ---------------------------------------------------------------------------------------------------------- linear models
def _lin_logjoint(B, G, logp, values, chunk=4096):
    """(l (N, S), states (S, H)) over all K^H states in index order (digit h of the index is k_h, low digit first)."""
    B, G, logp, values = _ld(B), _ld(G), _ld(logp), _ld(values)
    H, K = logp.shape
    S = K ** H
    ls, ss = [], []
    for c0 in range(0, S, chunk):
        idx = np.arange(c0, min(S, c0 + chunk), dtype=np.int64)
        dig = (idx[:, None] // (K ** np.arange(H, dtype=np.int64))[None, :]) % K
        s = values[dig]                                                   # (c, H)
        pr = np.zeros(len(idx), dtype=LD)
        for h in range(H):
            pr = pr + logp[h, dig[:, h]]
        quad = np.einsum("ch,hl,cl->c", s, G, s)
        ls.append(pr[None, :] - LD(0.5) * quad[None, :] + B @ s.T)
        ss.append(s)
    return np.concatenate(ls, axis=1), np.concatenate(ss, axis=0)


def lin_prep(Y, ymu, P):
    X = _ld(Y) - (LD(0) if ymu is None else _ld(ymu)[None, :])
    return X @ _ld(P), (X * X).sum(axis=1)


def lin_rows(Y, ymu, P, G, logp, values, cst, qcoef):
    """v_n = log sum_s exp(sum_h logp[h, k_h] - 1/2 s^T G s + x_n^T P s) + cst + qcoef |x_n|^2, x = y - ymu."""
    B, q = lin_prep(Y, ymu, P)
    l, _ = _lin_logjoint(B, G, logp, values)
    return lse_rows(l)[0] + LD(cst) + LD(qcoef) * q


def lin_means(Y, ymu, P, G, logp, values):
    """E_n[s] (N, H) under the posterior of the same log-joint."""
    B, _ = lin_prep(Y, ymu, P)
    l, s = _lin_logjoint(B, G, logp, values)
    return lse_rows(l)[1] @ s


def _check_blocks(blocks, H, A):
    assert sorted(h for b in blocks for h in b) == list(range(H)), blocks
    mask = np.zeros((H, H), dtype=bool)
    for b in blocks:
        mask[np.ix_(b, b)] = True
    assert not np.any(np.asarray(A)[~mask] != 0), "the couplings leave the blocks"


def lin_block_rows(Y, ymu, P, G, logp, values, cst, qcoef, blocks):
    """lin_rows for G that couples latents only inside `blocks` (lists of latent indices that partition 0..H-1): the log of a
    product of per-block sums."""
    logp = _ld(logp)
    _check_blocks(blocks, logp.shape[0], G)
    B, q = lin_prep(Y, ymu, P)
    v = LD(cst) + LD(qcoef) * q
    for b in blocks:
        l, _ = _lin_logjoint(B[:, b], _ld(G)[np.ix_(b, b)], logp[b], values)
        v = v + lse_rows(l)[0]
    return v


def lin_block_means(Y, ymu, P, G, logp, values, blocks):
    logp = _ld(logp)
    _check_blocks(blocks, logp.shape[0], G)
    B, _ = lin_prep(Y, ymu, P)
    E = np.zeros(B.shape, dtype=LD)
    for b in blocks:
        l, s = _lin_logjoint(B[:, b], _ld(G)[np.ix_(b, b)], logp[b], values)
        E[:, b] = lse_rows(l)[1] @ s
    return E


# ------------------------------------------------------------------------------------------------------------ MCA / MMCA
def _mca_pow(t, inv_rho, signed):
    with np.errstate(invalid="ignore"):
        return np.sign(t) * np.abs(t) ** LD(inv_rho) if signed else t ** LD(inv_rho)


def _mca_logjoint(Y, Wrho, inv_rho, signed, lp1, lp0, inv_s2):
    """(l (N, 2^H), Wbar (2^H, D)): the state index is the bit mask of s, causes added in ascending h, Wbar(0) = 0."""
    Y, Wrho = _ld(Y), _ld(Wrho)
    H, D = Wrho.shape
    wb = np.zeros((1 << H, D), dtype=LD)
    lp = np.zeros(1 << H, dtype=LD)
    for st in range(1 << H):
        k = bin(st).count("1")
        lp[st] = (k * LD(lp1) if k else LD(0)) + ((H - k) * LD(lp0) if H - k else LD(0))
        if st:
            t = np.zeros(D, dtype=LD)
            for h in range(H):
                if (st >> h) & 1:
                    t = t + Wrho[h]
            wb[st] = _mca_pow(t, inv_rho, signed)
    e = Y @ wb.T - LD(0.5) * (wb * wb).sum(axis=1)[None, :]
    with np.errstate(invalid="ignore"):
        l = np.where(lp[None, :] == -np.inf, -LD("inf"), lp[None, :] + LD(inv_s2) * e)
    return l, wb


def mca_rows(Y, Wrho, inv_rho, signed, lp1, lp0, inv_s2, cst):
    """v_n = log sum_s exp(|s| lp1 + (H - |s|) lp0 + inv_s2 (y^T Wbar(s) - 1/2 |Wbar(s)|^2)) + cst - inv_s2 / 2 |y_n|^2."""
    l, _ = _mca_logjoint(Y, Wrho, inv_rho, signed, lp1, lp0, inv_s2)
    return lse_rows(l)[0] + LD(cst) - LD(0.5) * LD(inv_s2) * (_ld(Y) ** 2).sum(axis=1)


def mca_means(Y, Wrho, inv_rho, signed, lp1, lp0, inv_s2):
    """Yhat_n = sum_s q_n(s) Wbar(s) (N, D)."""
    l, wb = _mca_logjoint(Y, Wrho, inv_rho, signed, lp1, lp0, inv_s2)
    return lse_rows(l)[1] @ wb


def _mca_disjoint(Y, Wrho, inv_rho, signed, lp1, lp0, inv_s2):
    Y, Wrho = _ld(Y), _ld(Wrho)
    assert np.all((Wrho != 0).sum(axis=0) <= 1), "a dimension has two causes"
    w = _mca_pow(Wrho, inv_rho, signed)                                  # (H, D): cause h alone
    on = LD(lp1) + LD(inv_s2) * (Y @ w.T - LD(0.5) * (w * w).sum(axis=1)[None, :])      # (N, H)
    off = np.full(on.shape, LD(lp0))
    with np.errstate(invalid="ignore"):
        both = np.logaddexp(on, off)
        q = np.where(both == -np.inf, LD(0), np.exp(on - np.where(both == -np.inf, LD(0), both)))
    return both, q, w


def mca_disjoint_rows(Y, Wrho, inv_rho, signed, lp1, lp0, inv_s2, cst):
    """mca_rows where every dimension d has at most one cause with Wrho[h, d] != 0: the causes are independent given y."""
    both, _, _ = _mca_disjoint(Y, Wrho, inv_rho, signed, lp1, lp0, inv_s2)
    return both.sum(axis=1) + LD(cst) - LD(0.5) * LD(inv_s2) * (_ld(Y) ** 2).sum(axis=1)


def mca_disjoint_means(Y, Wrho, inv_rho, signed, lp1, lp0, inv_s2):
    _, q, w = _mca_disjoint(Y, Wrho, inv_rho, signed, lp1, lp0, inv_s2)
    return q @ w


# -------------------------------------------------------------------------------------------------------------------- GSC
def cholesky(A):
    """Lower Cholesky factor in longdouble, column by column; a pivot that is not positive leaves NaN from there on."""
    A = np.array(A, dtype=LD)
    k = A.shape[0]
    L = np.zeros((k, k), dtype=LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(k):
            d = A[j, j]
            for p in range(j):
                d = d - L[j, p] * L[j, p]
            L[j, j] = np.sqrt(d)
            for i in range(j + 1, k):
                t = A[i, j]
                for p in range(j):
                    t = t - L[i, p] * L[j, p]
                L[i, j] = t / L[j, j]
    return L


def solve_lower(L, B):
    """L^-1 B by forward substitution."""
    L, B = _ld(L), np.array(B, dtype=LD)
    X = np.zeros(B.shape, dtype=LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(L.shape[0]):
            t = B[i]
            for p in range(i):
                t = t - L[i, p] * X[p]
            X[i] = t / L[i, i]
    return X


def _gsc_logjoint(U, M, Psi, mu, logp):
    """(l (N, 2^H), kap: per support (latents, (N, k) E[z_s | s, y_n])) from u_n = W^T Sigma^-1 y_n (the rows of U):
    l = kappa_s + mu_s^T u_s + 1/2 |A_s (u_s - m_s)|^2, A_s = Lk^-1 Lp^T, Psi_ss = Lp Lp^T, I + Lp^T M_ss Lp = Lk Lk^T,
    m_s = M_ss mu_s, kappa_s = log prior - sum log diag Lk - 1/2 mu_s^T m_s; E[z_s | s, y] = mu_s + A_s^T A_s (u_s - m_s)."""
    U, M, Psi, mu, logp = _ld(U), _ld(M), _ld(Psi), _ld(mu), _ld(logp).reshape(-1, 2)
    N, H = U.shape
    l = np.empty((N, 1 << H), dtype=LD)
    kap = []
    for st in range(1 << H):
        a = [h for h in range(H) if (st >> h) & 1]
        lp = LD(0)
        for h in range(H):
            lp = lp + logp[h, (st >> h) & 1]
        if lp == -np.inf:
            l[:, st] = -LD("inf")
            kap.append((a, np.zeros((N, len(a)), dtype=LD)))
            continue
        if not a:
            l[:, st] = lp
            kap.append((a, np.zeros((N, 0), dtype=LD)))
            continue
        Mss, mus = M[np.ix_(a, a)], mu[a]
        Lp = cholesky(Psi[np.ix_(a, a)])
        Lk = cholesky(np.eye(len(a), dtype=LD) + Lp.T @ Mss @ Lp)
        A = solve_lower(Lk, Lp.T)
        ms = Mss @ mus
        with np.errstate(invalid="ignore", divide="ignore"):
            kappa = lp - np.log(np.diag(Lk)).sum() - LD(0.5) * (mus * ms).sum()
        beta = U[:, a] - ms[None, :]
        z = beta @ A.T
        l[:, st] = kappa + U[:, a] @ mus + LD(0.5) * (z * z).sum(axis=1)
        kap.append((a, mus[None, :] + z @ A))
    return l, kap


def gsc_quad(Y, wdiag, Lw):
    """y^T Sigma^-1 y: sum_d wdiag_d y_d^2 (NULL: 1), or |Lw y|^2 with Lw lower."""
    Y = _ld(Y)
    if Lw is not None:
        assert wdiag is None
        Z = Y @ np.tril(_ld(Lw)).T
        return (Z * Z).sum(axis=1)
    return (Y * Y * (LD(1) if wdiag is None else _ld(wdiag)[None, :])).sum(axis=1)


def gsc_rows(Y, P, wdiag, Lw, M, Psi, mu, logp, cst):
    """v_n = log sum_s exp l_n(s) + cst - 1/2 y_n^T Sigma^-1 y_n."""
    l, _ = _gsc_logjoint(_ld(Y) @ _ld(P), M, Psi, mu, logp)
    return lse_rows(l)[0] + LD(cst) - LD(0.5) * gsc_quad(Y, wdiag, Lw)


def _gsc_means_from(l, kap, H):
    v, q = lse_rows(l)
    E = np.zeros((l.shape[0], H), dtype=LD)
    for st, (a, k) in enumerate(kap):
        if a:
            with np.errstate(invalid="ignore"):
                E[:, a] += np.where(q[:, st:st + 1] == 0, LD(0), q[:, st:st + 1] * k)
    E[np.isnan(v)] = LD("nan")
    return E


def gsc_means(Y, P, M, Psi, mu, logp):
    """E_n[s o z] (N, H) = sum_s q_n(s) E[z_s | s, y_n] (0 outside s)."""
    l, kap = _gsc_logjoint(_ld(Y) @ _ld(P), M, Psi, mu, logp)
    return _gsc_means_from(l, kap, _ld(M).shape[0])


def gsc_block_rows(Y, P, wdiag, Lw, M, Psi, mu, logp, cst, blocks):
    """gsc_rows for M and Psi that couple latents only inside `blocks`: kappa_s, mu_s^T u_s and |A_s beta|^2 are sums over
    the blocks."""
    logp = _ld(logp).reshape(-1, 2)
    H = logp.shape[0]
    _check_blocks(blocks, H, M)
    _check_blocks(blocks, H, Psi)
    U = _ld(Y) @ _ld(P)
    v = LD(cst) - LD(0.5) * gsc_quad(Y, wdiag, Lw)
    for b in blocks:
        l, _ = _gsc_logjoint(U[:, b], _ld(M)[np.ix_(b, b)], _ld(Psi)[np.ix_(b, b)], _ld(mu)[b], logp[b])
        v = v + lse_rows(l)[0]
    return v


def gsc_block_means(Y, P, M, Psi, mu, logp, blocks):
    logp = _ld(logp).reshape(-1, 2)
    H = logp.shape[0]
    _check_blocks(blocks, H, M)
    _check_blocks(blocks, H, Psi)
    U = _ld(Y) @ _ld(P)
    E = np.zeros(U.shape, dtype=LD)
    for b in blocks:
        l, kap = _gsc_logjoint(U[:, b], _ld(M)[np.ix_(b, b)], _ld(Psi)[np.ix_(b, b)], _ld(mu)[b], logp[b])
        E[:, b] = _gsc_means_from(l, kap, len(b))
    return E


# ------------------------------------------------------------------------------------------------------- the total's order
def total_fixed_order(rows):
    """total[0] of the returned rows in float64: thread t of 256 adds rows t, t + 256, ... in order (from 0.0), then thread t
    takes t + o for o = 128, 64, ..., 1."""
    rows = np.asarray(rows, dtype=np.float64)
    red = np.zeros(256, dtype=np.float64)
    for t in range(256):
        acc = np.float64(0.0)
        for x in rows[t::256]:
            acc = acc + x
        red[t] = acc
    o = 128
    while o > 0:
        red[:o] = red[:o] + red[o:2 * o]
        o //= 2
    return red[0]


# ------------------------------------------------------------------------------------------------------------------ plans
def lin_split(K, H):
    """(L, CH): the most low digits with K^L <= 1024 lo states (four per thread of 256), at most H."""
    L, CH = 0, 1
    while L < H and CH * K <= 1024:
        CH *= K
        L += 1
    return L, CH


def _space(kind, K, H):
    """(code, L, CH, space, loglik units) of the kind's state space, or the refusal of the bounds."""
    if kind == LIN:
        if not 2 <= K <= 8:
            return PM_EINVAL, 0, 0, 0, 0
        if H > 32 or K ** H > 2 ** 32:
            return PM_ERANGE, 0, 0, 0, 0
        L, CH = lin_split(K, H)
        return PM_OK, L, CH, K ** (H - L), K ** (H - L)
    if kind == MCA:
        return (PM_ERANGE, 0, 0, 0, 0) if H > 32 else (PM_OK, 0, 1, 2 ** H, -(-2 ** H // 1024))
    if kind == GSC:
        return (PM_ERANGE, 0, 0, 0, 0) if H > 16 else (PM_OK, 0, 1, 2 ** H, -(-2 ** H // 32))
    return PM_EINVAL, 0, 0, 0, 0


def loglik_plan(kind, N, D, K, H):
    """pm_loglik_exact_plan: (code, out) from the header's description."""
    if N < 0 or D < 1 or H < 1:
        return PM_EINVAL, None
    rc, L, CH, space, units = _space(kind, K, H)
    if rc:
        return rc, None
    tn = {LIN: 8 if N >= 64 else 1, MCA: 4 if N >= 16 else 1, GSC: 64}[kind]
    tiles = -(-N // tn)
    R = 1 if tiles == 0 else min(units, min(4096, -(-4096 // tiles)))
    return PM_OK, [tn, L, CH, space, units, R, tiles * R, N * (H + 2), 2 * N * R, 0]


def recon_plan(kind, N, D, K, H):
    """pm_recon_exact_plan: (code, out) from the header's description."""
    if N < 0 or D < 1 or H < 1:
        return PM_EINVAL, None
    rc, L, CH, space, _ = _space(kind, K, H)
    if rc:
        return rc, None
    if kind == LIN and H - L > 24:           # (no K in 2..8 reaches it inside 2^32 states: K = 2, H = 32 has 22 high digits)
        return PM_ERANGE, None
    if kind == MCA and D > 1024:
        return PM_ERANGE, None
    rows = 64 if kind == MCA else 256
    R = {LIN: min(256, max(1, space // 2)), MCA: min(64, max(1, space // 64)), GSC: min(256, max(1, space // 32))}[kind]
    nb = min(N, rows)
    width = D if kind == MCA else H
    return PM_OK, [rows, -(-N // rows), L, CH, space, R, -(-D // 64) if kind == MCA else 0,
                   nb if kind == MCA else nb * (H + 1), 2 * nb * R, nb * R * width]


def ranges(space, R):
    """The R ranges [space r / R, space (r + 1) / R) the kernels walk."""
    return [(space * r // R, space * (r + 1) // R) for r in range(R)]


# -------------------------------------------------------------------------------------------------------- operand builders
def lin_operands(rng, D, H, K, N, ymu=True, blocks=None, neg_inf=True, scale=0.6):
    """Operands of the linear entries that no model produces: non-integer values with a 0.0 among them, a different prior row
    per latent, one -inf prior entry, P and G unrelated to one another (G symmetric positive semi-definite, so that the
    sums stay bounded).  `blocks`: G couples latents inside the blocks only."""
    values = np.sort(rng.uniform(-1.5, 1.5, size=K))
    values[rng.randint(K)] = 0.0
    logp = np.log(rng.dirichlet(np.ones(K) * 2.0, size=H))
    if neg_inf:
        logp[rng.randint(H), rng.randint(K)] = -np.inf
    A = rng.normal(size=(D + 2, H)) * scale
    G = A.T @ A
    if blocks is not None:
        mask = np.zeros((H, H), dtype=bool)
        for b in blocks:
            mask[np.ix_(b, b)] = True
        G = np.where(mask, G, 0.0)
    return dict(Y=rng.normal(size=(N, D)), ymu=rng.normal(size=D) * 0.3 if ymu else None, P=rng.normal(size=(D, H)) * scale,
                G=np.ascontiguousarray(G), logp=logp, values=values, K=K, cst=-9.0, qcoef=-0.4)


def mca_operands(rng, D, H, N, signed, lp1=np.log(0.3), lp0=np.log(0.7), disjoint=False):
    """Wrho = W^rho for rho = 1 / inv_rho; signed: entries of both signs chosen so that sums over causes cross zero."""
    inv_rho = 1.0 / 6.0 if signed else 1.0 / 21.0
    W = rng.uniform(-1.5, 1.5, size=(H, D)) if signed else rng.uniform(0.2, 1.5, size=(H, D))
    if disjoint:
        owner = np.arange(D) % H
        rng.shuffle(owner)
        W = np.where(owner[None, :] == np.arange(H)[:, None], W, 0.0)
    Wrho = np.sign(W) * np.abs(W) ** (1.0 / inv_rho)
    if signed and not disjoint and H >= 2:
        Wrho[1, 0] = -Wrho[0, 0] * (1 + 2.0 ** -30)          # t = W0 + W1 of dimension 0 is 2^-30 of either, negative side
        if H >= 3:
            Wrho[2, 0] = abs(Wrho[0, 0]) * 2.0 ** -29        # ... and positive again with the third cause
    return dict(Y=rng.normal(size=(N, D)) * 0.8, Wrho=Wrho, inv_rho=inv_rho, signed=int(signed), lp1=float(lp1), lp0=float(lp0),
                inv_s2=1.7, cst=-6.0)


def gsc_operands(rng, D, H, N, noise="none", blocks=None, pi_edge=True):
    """P, M, Psi, mu, logp and the y^T Sigma^-1 y operand of `noise` ("wdiag", "Lw", "none"); M and Psi symmetric positive
    definite and otherwise unrelated to P.  `pi_edge`: one pi_h = 0 and one pi_h = 1 (H >= 3)."""
    A, Q = rng.normal(size=(H + 2, H)) * 0.5, rng.normal(size=(H, H)) * 0.3
    M, Psi = A.T @ A + 0.1 * np.eye(H), Q @ Q.T + np.diag(rng.uniform(0.4, 1.2, size=H))
    if blocks is not None:
        mask = np.zeros((H, H), dtype=bool)
        for b in blocks:
            mask[np.ix_(b, b)] = True
        M, Psi = np.where(mask, M, 0.0), np.where(mask, Psi, 0.0)
    pi = rng.uniform(0.15, 0.6, size=H)
    with np.errstate(divide="ignore"):
        if pi_edge and H >= 3:
            pi[1], pi[H - 1] = 0.0, 1.0
        logp = np.stack([np.log(1 - pi), np.log(pi)], axis=1)
    Lw = np.tril(rng.normal(size=(D, D)) * 0.3) + np.eye(D) if noise == "Lw" else None
    if Lw is not None:
        Lw = Lw + np.triu(np.full((D, D), np.nan), 1)         # the strict upper triangle is never read
    return dict(Y=rng.normal(size=(N, D)), P=rng.normal(size=(D, H)) * 0.5, wdiag=rng.uniform(0.5, 2.0, size=D) if noise == "wdiag"
                else None, Lw=Lw, M=np.ascontiguousarray(M), Psi=np.ascontiguousarray(Psi), mu=rng.normal(size=H) * 0.5,
                logp=np.ascontiguousarray(logp), cst=-12.0)


def straddling_blocks(H, L):
    """Blocks of 2 and 3 latents that straddle the lo / hi boundary at L, among them {L-1, L, H-1}; the rest in pairs taken
    from the two ends, singles last."""
    assert 2 <= L and L + 2 <= H
    blocks = [[L - 1, L, H - 1]]
    left = [h for h in range(H) if h not in blocks[0]]
    lo, hi = [h for h in left if h < L], [h for h in left if h >= L]
    while lo and hi:
        b = [lo.pop(), hi.pop(0)]
        if len(blocks) % 2 == 0 and lo:
            b.append(lo.pop(0))
        blocks.append(sorted(b))
    rest = lo + hi
    blocks += [rest[i:i + 2] for i in range(0, len(rest), 2)]
    return blocks


# ------------------------------------------------------------------------------------------------------------- case tables
# Shared by the CPU module (which pins every literal cell to the plan exports, without a device) and the GPU module.
# Linear models: (K, H) -> (L, CH, chunks).  NH = H - L >= 2 in the first seven; H <= L (one chunk, no high digit) in the rest.
LIN_CELLS = {
    (2, 12): (10, 1024, 4), (3, 8): (6, 729, 9), (4, 7): (5, 1024, 16), (5, 6): (4, 625, 25), (6, 5): (3, 216, 36),
    (7, 5): (3, 343, 49), (8, 5): (3, 512, 64),
    (2, 1): (1, 2, 1), (2, 3): (3, 8, 1), (8, 1): (1, 8, 1), (8, 3): (3, 512, 1),
}
LIN_LOGLIK_N = (1, 63, 64, 65, 71)              # ex_lin_tn: 1 below 64, 8 from 64; 65 and 71 leave a ragged tile of 1 and 7
LIN_RECON_N = (1, 255, 256, 257)                # the host walk's 256-row blocks
MCA_H = (1, 6, 11)
MCA_LOGLIK_N = (1, 15, 16, 17, 18)              # ex_mca_tn: 1 below 16, 4 from 16
MCA_RECON_N = (63, 64, 65)                      # 64-row blocks
MCA_RECON_D = (1, 63, 64, 65, 128)              # 64-wide slabs
GSC_H = (1, 5, 9)
GSC_N = (1, 63, 64, 65, 130)                    # 64-lane tiles
# Depth with couplings: (K, H) -> (L, CH, chunks, loglik R at N = 2, recon R)
LIN_DEPTH = {(2, 22): (10, 1024, 4096, 2048, 256), (3, 14): (6, 729, 6561, 2048, 256), (8, 8): (3, 512, 32768, 2048, 256)}
LIN_BOUND = {(2, 32): (10, 1024, 1 << 22, 2048), (3, 20): (6, 729, 3 ** 14, 2048), (4, 16): (5, 1024, 1 << 22, 2048)}
# Range cells (unit, kind, N, K, H) -> (R, units or space that caps it): R = 1, R = cap, 1 < R < cap
RANGE_CELLS = {
    ("loglik", LIN, 1, 2, 3): (1, 1), ("loglik", LIN, 1, 2, 12): (4, 4), ("loglik", LIN, 2, 2, 22): (2048, 4096),
    ("loglik", MCA, 1, 0, 6): (1, 1), ("loglik", MCA, 1, 0, 11): (2, 2), ("loglik", MCA, 32, 0, 20): (512, 1024),
    ("loglik", GSC, 1, 0, 5): (1, 1), ("loglik", GSC, 1, 0, 9): (16, 16), ("loglik", GSC, 600, 0, 14): (410, 512),
    ("recon", LIN, 1, 2, 3): (1, 1), ("recon", LIN, 1, 2, 12): (2, 4), ("recon", LIN, 2, 2, 22): (256, 4096),
    ("recon", MCA, 1, 0, 6): (1, 64), ("recon", MCA, 1, 0, 11): (32, 2048), ("recon", MCA, 2, 0, 20): (64, 1 << 20),
    ("recon", GSC, 1, 0, 5): (1, 32), ("recon", GSC, 1, 0, 9): (16, 512), ("recon", GSC, 2, 0, 14): (256, 1 << 14),
}
