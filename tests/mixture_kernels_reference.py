"""Plain NumPy reference (np.longdouble, no torch, no library, no numpy.linalg) of the mixture kernels (mixture_kernels.hip),
operand for operand as include/prosper_hip.h and the header comment of mixture_kernels.hip state the nine pm_mix_* entries.

  scores        logpj = (S + c) coef + lp, S = (rs o Y) Bl^T (+ (Y o Y) Bq^T), with the sum of magnitudes of the terms of every S
  f64_pattern   a longdouble result with the non-finite values float64 arithmetic gives (a sum past DBL_MAX is +-inf there)
  posterior     the row epilogue: exp, NaN -> tiny, < tiny -> tiny, inf -> DBL_MAX / H, divided by the row sum
  loglik_rows   log sum_h exp(z_nh): any NaN -> NaN, else any +inf -> +inf, all -inf -> -inf; minus sum_d lgamma(rs_n y_nd + yoff + 1)
                when pmf.  The argument is formed in float64 exactly as the kernel forms it (IEEE: the same bits), lgamma is
                math.lgamma per element in float64, and the D values are summed in longdouble.
  chol          left-looking Cholesky of the LOWER triangle (the upper one is never read): L, L^-1, log det, status; the first
                pivot that is not a positive finite number ends it with status 1
  maha          S[n,h] = |B_h u|^2 (mode 0 / None) or u . (B_h u) (mode 1: B_h = Sinv_h^T), u = y_n - w_h, with z = B_h u and the
                sums of magnitudes the bounds need
  mstats        [colsum P (H) | Y^T P (D, H) | kind 1: (Y o Y)^T P (D, H) | kind 2: Y^T diag(P[:, h]) Y (H, D, D)] and the sum of
                magnitudes of the terms of every entry
  stats_len, stats_chunks, chunk_rows, work_len: restated from the header text and the launcher's comment

CASES holds one literal shape tuple per edge the GPU module (tests/test_mixture_kernels_gpu.py) covers; make_case(name, exact)
builds the operands.  exact=True: small integers, powers of two and dyadic fractions, chosen so that every product and every
partial sum in ANY order is a float64 (asserted here: sum of magnitudes x 2^(fractional bits) < 2^53).  exact=False: magnitudes
in [0.5, 2] with mixed signs (cancellation), |c| <= 0.25.  tests/test_mixture_kernels_cpu.py pins this file against the
committed reference outputs (tests/golden/mixture_step_*.npz) and asserts what the GPU module relies on."""
import math

import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
TINY = 2.2250738585072014e-308
DBL_MAX = 1.7976931348623157e308
PM_MAX_H = 1024
BT, BK = 64, 16                         # output tile edge and K step of mixture_kernels.hip
KIND_MOP, KIND_DIAG, KIND_FULL = 0, 1, 2
BIG = 1e308                             # x 1e10 is past DBL_MAX: one such term makes a float64 sum +-inf, whatever the order


# ----------------------------------------------------------------------------------------------------------- host-only
def cdiv(a, b):
    return -(-a // b)


def stats_len(D, H, kind):
    if D <= 0 or H <= 0 or kind not in (0, 1, 2):
        return -1
    return H + D * H + (D * H if kind == 1 else H * D * D if kind == 2 else 0)


def stats_chunks(N, D, H, kind):
    """About 1024 workgroups in the Y^T P launch, chunks of at least 256 datapoints, at most 64 partials, the workspace at most
    2^27 doubles, and G H within grid z for the Gram launch."""
    if N <= 0 or D <= 0 or H <= 0 or kind not in (0, 1, 2):
        return -1
    G = cdiv(1024, cdiv(D, BT) * cdiv(H, BT))
    G = min(G, max(1, N // 256))
    G = min(G, max(1, (1 << 27) // stats_len(D, H, kind)))
    if kind == 2:
        G = min(G, max(1, 65535 // H))
    return max(1, min(G, 64))


def chunk_rows(N, G):
    """Rows per chunk: ceil(N / G) rounded up to the K step."""
    return cdiv(cdiv(N, G), BK) * BK


def work_len(N, D, H, kind):
    G, L = stats_chunks(N, D, H, kind), stats_len(D, H, kind)
    return -1 if G < 0 or L < 0 else G * L


def chunk_layout(N, D, H, kind):
    """(G, chunk, rows of every chunk): chunk g holds rows [g chunk, min(N, (g + 1) chunk)), none when it starts past N."""
    G = stats_chunks(N, D, H, kind)
    ch = chunk_rows(N, G)
    return G, ch, [max(0, min(N, (g + 1) * ch) - g * ch) for g in range(G)]


# ------------------------------------------------------------------------------------------------------------- scores
def f64_pattern(x):
    """`x` (longdouble) with the entries float64 cannot hold as finite numbers replaced by what float64 holds (+-inf, NaN)."""
    x = np.asarray(x, dtype=LD)
    with np.errstate(over="ignore", invalid="ignore"):
        f = x.astype(np.float64)
    return np.where(np.isfinite(f), x, f.astype(LD))


def scores(Y, rs, Bq, Bl, c, coef, lp):
    """(logpj, S, mag): mag[n,h] = sum_d |rs_n y_nd| |Bl[h,d]| (+ y_nd^2 |Bq[h,d]|), the terms of S[n,h]."""
    with np.errstate(all="ignore"):
        A = np.asarray(Y, dtype=LD)
        if rs is not None:
            A = A * np.asarray(rs, dtype=LD)[:, None]
        Bl = np.asarray(Bl, dtype=LD)
        S = A @ Bl.T
        mag = np.abs(A) @ np.abs(Bl).T
        if Bq is not None:
            Bq = np.asarray(Bq, dtype=LD)
            S = S + (A * A) @ Bq.T
            mag = mag + (A * A) @ np.abs(Bq).T
        S = f64_pattern(S)
        logpj = f64_pattern((S + np.asarray(c, dtype=LD)[None, :]) * LD(coef) + np.asarray(lp, dtype=LD)[None, :])
    return logpj, S, mag


def logpj_of(S, c, coef, lp):
    """pm_mix_posterior_f64's first half: (S + c) coef + lp from a given S."""
    with np.errstate(all="ignore"):
        S, c, lp = np.asarray(S, dtype=LD), np.asarray(c, dtype=LD), np.asarray(lp, dtype=LD)
        return f64_pattern((S + c[None, :]) * LD(coef) + lp[None, :])


def posterior(logpj):
    """exp(logpj) with no max subtraction, NaN -> tiny, < tiny -> tiny, inf -> DBL_MAX / H, divided by the row sum."""
    z = np.asarray(logpj, dtype=LD)
    H = z.shape[1]
    with np.errstate(all="ignore"):
        p = np.exp(z)
        p = np.where(p > LD(DBL_MAX), LD(np.inf), p)          # float64's exp overflows there
        p = np.where(np.isnan(p), LD(TINY), p)
        p = np.where(p < LD(TINY), LD(TINY), p)
        p = np.where(np.isinf(p), LD(DBL_MAX) / H, p)
    return p / p.sum(axis=1)[:, None]


def lgamma_rows(Y, rs, yoff):
    """(sum_d lgamma(x_nd), sum_d |lgamma(x_nd)|), x = rs_n y_nd + yoff + 1 formed in float64 as the kernel does; math.lgamma per
    element in float64, summed in longdouble.  A NaN argument gives NaN."""
    Y = np.asarray(Y, dtype=np.float64)
    with np.errstate(all="ignore"):
        x = (Y * (np.ones(Y.shape[0]) if rs is None else np.asarray(rs, dtype=np.float64))[:, None] + np.float64(yoff)) + 1.0
    tot = np.zeros(Y.shape[0], dtype=LD)
    mag = np.zeros(Y.shape[0], dtype=LD)
    for n in range(Y.shape[0]):
        for v in x[n]:
            g = LD(math.lgamma(v)) if np.isfinite(v) and v > 0 else LD(np.nan) if np.isnan(v) else LD(np.inf)
            tot[n] += g
            mag[n] += abs(g)
    return tot, mag


def loglik_rows(logpj, Y=None, rs=None, pmf=0, yoff=0.0):
    """(rows, lse, lgamma magnitude): log sum_h exp(z_nh) with the kernel's conventions, minus the row term when pmf."""
    z = np.asarray(logpj, dtype=LD)
    N = z.shape[0]
    lse = np.zeros(N, dtype=LD)
    with np.errstate(all="ignore"):
        for n in range(N):
            r = z[n]
            if np.isnan(r).any():
                lse[n] = np.nan
            elif np.isposinf(r).any():
                lse[n] = np.inf
            elif np.isneginf(r).all():
                lse[n] = -np.inf
            else:
                m = r.max()
                lse[n] = m + np.log(np.exp(r - m).sum())
        if not pmf:
            return lse, lse, np.zeros(N, dtype=LD)
        lg, lgmag = lgamma_rows(Y, rs, yoff)
        return lse - lg, lse, lgmag


# --------------------------------------------------------------------------------------------------------------- chol
def chol(S):
    """Left-looking longdouble Cholesky of the lower triangle of one D x D matrix (float64; the upper triangle is not read):
    (L, Linv, logdet, status).  status 1, logdet NaN (L, Linv as far as they got) at the first pivot that is not a positive
    finite number."""
    A = np.asarray(S, dtype=np.float64)
    D = A.shape[0]
    L = np.zeros((D, D), dtype=LD)
    ld = LD(0)
    with np.errstate(all="ignore"):
        for j in range(D):
            d = LD(A[j, j]) - (L[j, :j] * L[j, :j]).sum()
            if not (d > 0) or not np.isfinite(np.float64(d)):
                return L, np.zeros((D, D), dtype=LD), LD(np.nan), 1
            ld += np.log(d)
            ljj = np.sqrt(d)
            L[j, j] = ljj
            if j + 1 < D:
                L[j + 1:, j] = (A[j + 1:, j].astype(LD) - L[j + 1:, :j] @ L[j, :j]) / ljj
        X = np.zeros((D, D), dtype=LD)
        for i in range(D):                              # row i of L^-1 by forward substitution
            e = np.zeros(D, dtype=LD)
            e[i] = 1
            X[i] = (e - L[i, :i] @ X[:i]) / L[i, i]
    return L, X, ld, 0


def spectral_cond(A, iters=200):
    """cond_2 of a symmetric positive definite matrix by power iteration on A and on A^-1 = Linv^T Linv (no numpy.linalg)."""
    A = np.asarray(A, dtype=LD)
    A = np.tril(A) + np.tril(A, -1).T
    _, X, _, status = chol(A.astype(np.float64))
    assert status == 0
    Ainv = X.T @ X
    out = []
    for M in (A, Ainv):
        v = np.ones(M.shape[0], dtype=LD) + LD(0.01) * np.arange(M.shape[0])
        lam = LD(0)
        for _ in range(iters):
            w = M @ v
            lam = np.sqrt((w * w).sum() / (v * v).sum())
            v = w / np.abs(w).max()
        out.append(lam)
    return float(out[0] * out[1]) * 1.05                # (power iteration approaches from below)


# --------------------------------------------------------------------------------------------------------------- maha
def maha(Y, W, B, mode):
    """(S (N, H), Z (N, H, D) = B_h u, Zmag = |B_h| |u|, Uu = |u|): mode[h] == 0 / mode None: S = sum_j z_j^2; mode[h] == 1:
    S = sum_j z_j u_j (B_h = Sinv_h^T)."""
    Y, W, B = np.asarray(Y, dtype=LD), np.asarray(W, dtype=LD), np.asarray(B, dtype=LD)
    N, D = Y.shape
    H = W.shape[0]
    with np.errstate(all="ignore"):
        u = Y[:, None, :] - W[None, :, :]                              # (N, H, D)
        Z = np.einsum("hjk,nhk->nhj", B, u)
        Zmag = np.einsum("hjk,nhk->nhj", np.abs(B), np.abs(u))
        S = np.zeros((N, H), dtype=LD)
        for h in range(H):
            sq = mode is None or int(mode[h]) == 0
            S[:, h] = (Z[:, h] * Z[:, h]).sum(axis=1) if sq else (Z[:, h] * u[:, h]).sum(axis=1)
    return S, Z, Zmag, np.abs(u)


# ------------------------------------------------------------------------------------------------------------- mstats
def mstats(Y, P, rs, kind):
    """(stats, mag) in the packed layout of pm_mix_stats_len; rs scales the rows of Y in Y^T P (kind 0 only)."""
    Y, P = np.asarray(Y, dtype=LD), np.asarray(P, dtype=LD)
    N, D = Y.shape
    H = P.shape[1]
    assert rs is None or kind == KIND_MOP
    A = Y if rs is None else Y * np.asarray(rs, dtype=LD)[:, None]
    parts = [(P.sum(axis=0), np.abs(P).sum(axis=0)), ((A.T @ P).reshape(-1), (np.abs(A).T @ np.abs(P)).reshape(-1))]
    if kind == KIND_DIAG:
        parts.append((((Y * Y).T @ P).reshape(-1), ((Y * Y).T @ np.abs(P)).reshape(-1)))
    if kind == KIND_FULL:
        parts.append((np.einsum("nm,nh,nj->hmj", Y, P, Y).reshape(-1),
                      np.einsum("nm,nh,nj->hmj", np.abs(Y), np.abs(P), np.abs(Y)).reshape(-1)))
    st, mag = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    assert len(st) == stats_len(D, H, kind)
    return st, mag


# --------------------------------------------------------------------------------------------------------------- cases
# The three forms of the scores kernel: MoG diagonal (Bq given), MoP, MoP with the row scale.
FORMS = ("mog", "mop", "mop_rs")
# pm_mix_loglik_f64: (form, pmf, yoff)
LL_FORMS = (("mog", 0, 0.0), ("mop", 0, 0.0), ("mop", 1, 0.0), ("mop_rs", 1, 1.0), ("mop_rs", 0, 0.0))
# the scores shapes: each value of N in {1, 63, 64, 65, 130}, D in {1, 15, 16, 17, 33}, H in {1, 63, 64, 65, 130} with the middle value
# of the other two, and H = PM_MAX_H once
CASES = {
    # name: (entry, N, D, H)
    "s_n1": ("scores", 1, 16, 64), "s_n63": ("scores", 63, 16, 64), "s_mid": ("scores", 64, 16, 64), "s_n65": ("scores", 65, 16, 64),
    "s_n130": ("scores", 130, 16, 64), "s_d1": ("scores", 64, 1, 64), "s_d15": ("scores", 64, 15, 64), "s_d17": ("scores", 64, 17, 64),
    "s_d33": ("scores", 64, 33, 64), "s_h1": ("scores", 64, 16, 1), "s_h63": ("scores", 64, 16, 63), "s_h65": ("scores", 64, 16, 65),
    "s_h130": ("scores", 64, 16, 130), "s_hmax": ("scores", 5, 3, 1024),
    # non-finite rows (row 1 NaN, 2 one +inf, 3 every z -inf, 4 -inf in all of the first H block) and the row maximum in block 2 of 3
    "s_special": ("scores", 65, 17, 130),
    # pm_mix_loglik_f64 only: above PM_MAX_H
    "l_h1100": ("loglik", 5, 3, 1100),
    # pm_mix_posterior_f64: (entry, N, 0, H)
    "p_n1_h1": ("posterior", 1, 0, 1), "p_n3_h64": ("posterior", 3, 0, 64), "p_n4_h65": ("posterior", 4, 0, 65),
    "p_n5_h1024": ("posterior", 5, 0, 1024), "p_n5_h1": ("posterior", 5, 0, 1), "p_n1_h1024": ("posterior", 1, 0, 1024),
    "p_n4_h64": ("posterior", 4, 0, 64), "p_n3_h65": ("posterior", 3, 0, 65),
    # pm_mix_chol_f64: (entry, 0, D, H)
    "c_d1": ("chol", 0, 1, 3), "c_d2": ("chol", 0, 2, 3), "c_d17": ("chol", 0, 17, 3), "c_d64": ("chol", 0, 64, 3),
    "c_d257": ("chol", 0, 257, 2), "c_d300": ("chol", 0, 300, 2),
    # pm_mix_maha_f64
    "m_n1": ("maha", 1, 64, 3), "m_mid": ("maha", 64, 64, 3), "m_n65": ("maha", 65, 64, 3), "m_d1": ("maha", 64, 1, 3),
    "m_d15": ("maha", 64, 15, 3), "m_d17": ("maha", 64, 17, 3), "m_d65": ("maha", 64, 65, 3), "m_d130": ("maha", 64, 130, 3),
    "m_h1": ("maha", 64, 64, 1), "m_n65_d130": ("maha", 65, 130, 3),
}
# pm_mix_mstats_f64: name -> (N, D, H, kinds, G, chunk, empty trailing chunks, rows of the last non-empty chunk)
# kinds: 0 = MoP, "0rs" = MoP with the row scale, 1 = MoG diagonal, 2 = MoG full
MSTATS_CASES = {
    "t_n1": (1, 5, 3, (0, "0rs", 1, 2), 1, 16, 0, 1),
    "t_n15": (15, 5, 3, (0, "0rs", 1, 2), 1, 16, 0, 15),
    "t_n16": (16, 5, 3, (0, "0rs", 1, 2), 1, 16, 0, 16),
    "t_n17": (17, 5, 3, (0, "0rs", 1, 2), 1, 32, 0, 17),
    "t_n255": (255, 5, 3, (0, "0rs", 1, 2), 1, 256, 0, 255),
    "t_g2": (600, 33, 40, (0, "0rs", 1), 2, 304, 0, 296),                 # the second chunk ends in a partial K step (296 = 18.5 x 16)
    "t_g2_full": (600, 6, 3, (2,), 2, 304, 0, 296),                      # kind 2, H = 3, G = 2: blockIdx.z carries both indices
    "t_g64": (16400, 4, 3, (0, "0rs", 1, 2), 64, 272, 3, 80),            # chunks 61 .. 63 start past N
    "t_d63_h65": (37, 63, 65, (0, "0rs", 1), 1, 48, 0, 37),              # tile edges; the column sum across two column tiles
    "t_d65_h63": (37, 65, 63, (0, "0rs", 1), 1, 48, 0, 37),
    "t_d65_h130": (37, 65, 130, (0, 1), 1, 48, 0, 37),
    "t_d63_full": (37, 63, 3, (2,), 1, 48, 0, 37),
    "t_d65_full": (37, 65, 3, (2,), 1, 48, 0, 37),
}
CHOL_FAILS = ("first", "middle", "last", "nan", "zero")
SPECIAL_ROWS = {"nan": 1, "pinf": 2, "all_ninf": 3, "block1_ninf": 4}
ISOLATION_ROWS = (0, 31, 64)            # tile positions of the NaN, +inf and 1e300 rows at N = 65


def _seed(*k):
    s = 17
    for v in k:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return np.random.RandomState(s)


def _ints(rng, shape, lo, hi):
    """Position-dependent integers in [lo, hi] as float64 (not symmetric: a transposed or shifted tile map changes the answer)."""
    shape = tuple(shape)
    a = rng.randint(0, hi - lo + 1, size=shape)
    pos = np.arange(int(np.prod(shape))).reshape(shape)
    return (lo + (a + pos % 5) % (hi - lo + 1)).astype(np.float64)


def _generic(rng, shape, signed=True):
    """Magnitudes in [0.5, 2], mixed signs."""
    v = rng.uniform(0.5, 2.0, size=shape)
    return v * rng.choice([-1.0, 1.0], size=shape) if signed else v


def is_multiple(x, bits):
    """Every entry of x is an integer multiple of 2^-bits."""
    v = np.asarray(x, dtype=LD) * LD(2.0) ** bits
    return bool((v == np.floor(v)).all())


def exact_ok(mag, bits):
    """Sums whose terms' magnitudes add up to `mag`, every term a multiple of 2^-bits, are float64 numbers in any order."""
    return bool((np.asarray(mag, dtype=LD) * LD(2.0) ** bits < LD(2.0) ** 53).all())


def scores_case(N, D, H, form, exact, pmf=0, special=False, seed=0):
    """Operands of pm_mix_scores_f64 / pm_mix_loglik_f64.  exact: Y integers in [-3, 3] ([0, 3] when pmf), rs in {1/2, 1, 2},
    Bl integers in [-2, 2], Bq multiples of 1/4 in [0, 1], c and lp multiples of 1/8, coef -1/2 (MoG) or 1/4 (MoP): every
    term of (S + c) coef + lp is a multiple of 2^-6.  Generic: magnitudes in [0.5, 2] with mixed signs, |c| <= 0.25,
    coef -0.75 / 0.8."""
    rng = _seed(N, D, H, FORMS.index(form), exact, pmf, special, seed)
    sq, scaled = form == "mog", form == "mop_rs"
    if exact:
        Y = _ints(rng, (N, D), 0 if pmf else -3, 3)
        Bl = _ints(rng, (H, D), -2, 2)
        Bq = _ints(rng, (H, D), 0, 4) / 4.0 if sq else None
        rs = rng.choice([0.5, 1.0, 2.0], size=N) if scaled else None
        c = _ints(rng, (H,), -8, 8) / 8.0
        lp = _ints(rng, (H,), -24, -1) / 8.0
        coef = -0.5 if sq else 0.25
    else:
        Y = _generic(rng, (N, D), signed=not pmf)
        Bl = _generic(rng, (H, D)) / (1.0 if sq else 2.0)
        Bq = _generic(rng, (H, D), signed=False) if sq else None
        rs = rng.uniform(0.5, 2.0, size=N) if scaled else None
        c = rng.uniform(-0.25, 0.25, size=H)
        lp = rng.uniform(-3.0, -0.5, size=H)
        coef = -0.75 if sq else 0.8
    case = dict(N=N, D=D, H=H, form=form, exact=exact, Y=Y, rs=rs, Bq=Bq, Bl=Bl, c=c, coef=coef, lp=lp, pmf=pmf, bits=6)
    if special:
        assert N >= 5 and D >= 4 and H > BT
        sg = 1.0 if coef > 0 else -1.0                 # so that the sign of z is the sign written below
        Y[:, :3] = 0.0
        Bl[:, :3] = 0.0
        if sq:
            Bq[:, :3] = 0.0
        Bl[7, 0] = sg * BIG                            # column 0: z[n, 7] = +inf for the row that has y_n0 = 1e10
        Bl[:, 1] = -sg * BIG                           # column 1: every z of the row -inf
        Bl[:BT, 2] = -sg * BIG                         # column 2: the first H block -inf, the others finite
        Y[SPECIAL_ROWS["nan"], D - 1] = np.nan
        Y[SPECIAL_ROWS["pinf"], 0] = 1e10
        Y[SPECIAL_ROWS["all_ninf"], 1] = 1e10
        Y[SPECIAL_ROWS["block1_ninf"], 2] = 1e10
        lp[BT + 6] += 3.0                              # the row maximum in the second of three H blocks (asserted on the CPU)
        case["special"] = True
    if exact and not special:
        _, _, mag = scores(Y, rs, Bq, Bl, c, coef, lp)
        total = (mag + np.abs(c)[None, :]) * abs(coef) + np.abs(lp)[None, :]
        assert exact_ok(total, case["bits"])
        assert all(is_multiple(v, b) for v, b in ((Y, 0), (Bl, 0), (c, 3), (lp, 3), (coef, 2))) and (not sq or is_multiple(Bq, 2))
        assert rs is None or is_multiple(rs, 1)
    return case


def posterior_case(N, H, exact, seed=0):
    """S (N, H) for pm_mix_posterior_f64; row 0 of a case with N >= 3 carries a NaN, a +inf and a -inf."""
    rng = _seed(N, H, exact, seed, 77)
    if exact:
        S, c, lp, coef = _ints(rng, (N, H), -40, 40) / 4.0, _ints(rng, (H,), -8, 8) / 8.0, _ints(rng, (H,), -24, -1) / 8.0, -0.5
    else:
        S = _generic(rng, (N, H)) * 8.0
        c, lp, coef = rng.uniform(-0.25, 0.25, size=H), rng.uniform(-3.0, -0.5, size=H), -0.75
    if N >= 3:
        S[0, 0] = np.nan
        S[0, H // 2] = np.inf if H > 1 else S[0, H // 2]          # coef < 0: z = -inf
        S[0, H - 1] = -np.inf if H > 2 else S[0, H - 1]           # z = +inf
        S[N - 1, :] = 2000.0                                      # every exp underflows: the row is 1 / H
    case = dict(N=N, H=H, exact=exact, S=S, c=c, lp=lp, coef=coef, bits=6)
    if exact:
        fin = np.where(np.isfinite(S), S, 0.0)
        assert exact_ok((np.abs(fin) + np.abs(c)[None, :]) * abs(coef) + np.abs(lp)[None, :], 6) and is_multiple(fin, 2)
    return case


def chol_case(D, H, fail=None, seed=0):
    """H covariances I + 0.3 B B^T / D (well conditioned); `fail` = (component, what): what in "first", "middle", "last" sets that
    pivot's diagonal entry to -1; "nan" puts a NaN into the lower triangle (the diagonal at D = 1); "zero" makes the component
    the identity with one off-diagonal 1 next to the LAST pivot, whose value is then EXACTLY 0 (1 - 1^2; at D = 1 the entry
    itself is 0): not positive, and not negative either.  (Accepting a zero pivot anywhere but last turns the rows below it
    into NaN and fails at the next pivot with the same outputs, so only the last pivot can show it.)  Returns the (H, D, D) float64 array, symmetric: the caller
    overwrites the strict upper triangle."""
    rng = _seed(D, H, seed, 91)
    S = np.empty((H, D, D))
    for h in range(H):
        B = rng.normal(size=(D, D)) / np.sqrt(D)
        S[h] = np.eye(D) + 0.3 * B @ B.T
        S[h] = np.tril(S[h]) + np.tril(S[h], -1).T
    pivot = None
    if fail is not None:
        h, what = fail
        pivot = {"first": 0, "middle": D // 2, "last": D - 1, "nan": min(D - 1, max(1, D // 2)), "zero": D - 1}[what]
        if what == "nan":
            S[h, pivot, 0 if D > 1 else pivot] = np.nan      # L[pivot, 0] is NaN, so pivot `pivot` is
        elif what == "zero":
            S[h] = np.eye(D)
            if D > 1:
                S[h, pivot, pivot - 1] = S[h, pivot - 1, pivot] = 1.0
            else:
                S[h, 0, 0] = 0.0
        else:
            S[h, pivot, pivot] = -1.0
    return S, pivot


def maha_case(N, D, H, exact, mode_kind, seed=0):
    """mode_kind: "null", "zeros" or "mixed" (component H // 2 in mode 1, with a non-symmetric B).  exact: integers -- Y, W in
    [-3, 3], B in [-2, 2]; |u| <= 6, |z| <= 12 D, sum z^2 <= 144 D^3 < 2^53."""
    rng = _seed(N, D, H, exact, seed, 55)
    if exact:
        Y, W, B = _ints(rng, (N, D), -3, 3), _ints(rng, (H, D), -3, 3), _ints(rng, (H, D, D), -2, 2)
    else:
        Y, W, B = _generic(rng, (N, D)), _generic(rng, (H, D)), _generic(rng, (H, D, D)) / np.sqrt(D)
    mode = None if mode_kind == "null" else np.zeros(H, dtype=np.int32)
    if mode_kind == "mixed":
        mode[H // 2] = 1
        if D > 1:
            assert not np.array_equal(B[H // 2], B[H // 2].T)
    case = dict(N=N, D=D, H=H, exact=exact, Y=Y, W=W, B=B, mode=mode, bits=0)
    if exact:
        assert exact_ok(144 * D ** 3, 0)
    return case


def mstats_case(N, D, H, kind, exact, seed=0):
    """kind in (0, "0rs", 1, 2).  exact: Y integers in [-3, 3], P multiples of 1/8 in [0, 1], rs in {1/2, 1, 2}: every term is a
    multiple of 2^-4.  Generic: Y magnitudes in [0.5, 2] with mixed signs, P in (0, 1), rs in [0.5, 2]."""
    rng = _seed(N, D, H, 3 if kind == "0rs" else kind, exact, seed, 33)
    scaled = kind == "0rs"
    k = KIND_MOP if scaled else int(kind)
    if exact:
        Y, P = _ints(rng, (N, D), -3, 3), _ints(rng, (N, H), 0, 8) / 8.0
        rs = rng.choice([0.5, 1.0, 2.0], size=N) if scaled else None
    else:
        Y, P = _generic(rng, (N, D)), rng.uniform(0.01, 1.0, size=(N, H))
        rs = rng.uniform(0.5, 2.0, size=N) if scaled else None
    case = dict(N=N, D=D, H=H, kind=k, exact=exact, Y=Y, P=P, rs=rs, bits=4)
    if exact:
        assert exact_ok(mstats(Y, P, rs, k)[1], 4) and is_multiple(P, 3) and is_multiple(Y, 0)
    return case


def make_case(name, exact, **kw):
    """Operands of a case of CASES or MSTATS_CASES.  Keywords: form / pmf (scores, loglik), mode_kind (maha), fail (chol),
    kind (mstats)."""
    if name in MSTATS_CASES:
        N, D, H = MSTATS_CASES[name][:3]
        return mstats_case(N, D, H, kw["kind"], exact)
    entry, N, D, H = CASES[name]
    if entry in ("scores", "loglik"):
        return scores_case(N, D, H, kw.get("form", "mop"), exact, kw.get("pmf", 0), special=name == "s_special")
    if entry == "posterior":
        return posterior_case(N, H, exact)
    if entry == "chol":
        return chol_case(D, H, kw.get("fail"))
    if entry == "maha":
        return maha_case(N, D, H, exact, kw.get("mode_kind", "mixed"))
    raise KeyError(name)


def isolation_rows(Y):
    """Y (65, D) with a NaN row, a +inf row and a 1e300 row at tile positions 0, 31 and 64."""
    Z = np.array(Y, dtype=np.float64)
    assert Z.shape[0] == 65
    Z[ISOLATION_ROWS[0]] = np.nan
    Z[ISOLATION_ROWS[1]] = np.inf
    Z[ISOLATION_ROWS[2]] = 1e300
    return Z
