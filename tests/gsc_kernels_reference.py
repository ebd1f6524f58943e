"""Plain NumPy reference (np.longdouble, no torch, no library) of the GSC kernels (gsc_kernels.hip) as include/prosper_hip.h
states them and oracle/gsc_oracle.py restates them, operand for operand as the C ABI takes them: scores = Y W, gram = W^T W,
psi_sq, ynorm2, the 8 (or 9) x H per-latent tables [c0 | c1 | gm | il | kl | ilam | mu | lpi | 1/sigma_sq, thr, thr_p] and the
16-bit state masks are float64 / integer INPUTS of the kernels, so the reference starts from the same tables and carries
everything behind them in longdouble.  No numpy.linalg: the g x g algebra is an explicit Gauss-Jordan in longdouble.

  component_scores   c0 - yn / s2 + c1 a + (a - gm)^2 il, then NaN / < -DBL_MAX (-inf too) -> -DBL_MAX, then +inf -> 0
  rank_values        the float64 score with its low 10 mantissa bits dropped: what the selection ranks on
  select             the H' largest ranking values, equal ones towards the larger latent index, sorted by index
  estep              every state's log-joint [null | singletons | multi-cause states in table order] and cancellation term, the
                     weights exp(beta lp) (NaN / < tiny -> tiny, null state unclamped), xpt_s, xpt_sz, the un-normalised
                     blocks of pm_gsc_estep_lpj_blocks_f64 and every datapoint's normalised pair blocks
  raw_stats          [U_ss strict upper | U_zz (with or without its diagonal) | cs | csz | dzz] by form, with the thr_p rule
  packed_stats       the layout of pm_gsc_pack_stats_f64
  list_split         the LIST form's lists (both value planes) and dense rows
  list_pairs         the two H x H products of pm_gsc_list_pairs_f64 from lists

CASES holds one smallest shape per dispatch cell of pm_gsc_plan as literal tuples; make_case(name, hot) builds its operands
directly as kernel inputs, HOT (all K = 1 + H + S weights of a row within a factor e) and COLD (states on both sides of
log(tiny), arguments inside the libm window [log(tiny), -708), rows in which every state underflows).
tests/test_gsc_kernels_cpu.py pins this file against oracle/gsc_oracle.py and asserts what the GPU module relies on."""
import itertools

import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
TINY = 2.2250738585072014e-308
LOG_TINY = -708.3964185322641          # log(TINY)
WINDOW_HI = -708.0                     # arguments in [LOG_TINY, WINDOW_HI) take libm in the kernel
DBL_MAX = 1.7976931348623157e308
NZ_MAX = 16                            # PM_BSC_NZ_MAX
XCD_COPIES = 8
ESTEP, LIST_PAIRS, PACK, COMPONENT_SCORES = 0, 1, 2, 3          # PM_GSC_PLAN_*
F_LPJ, F_BLOCKS, F_LISTS = 1, 2, 4
PLAIN, LACC, LPJ, LIST = 0, 1, 2, 3                             # PM_GSC_FORM_*
PLAN_LEN = 12
FORM_NAMES = {PLAIN: "plain", LACC: "lacc", LPJ: "lpj", LIST: "list"}


# ------------------------------------------------------------------------------------------------------------ shapes
def full_states(Hp, gamma):
    """Multi-cause states of the full table: sum_{g=2..gamma} C(H', g)."""
    S, c = 0, Hp
    for g in range(2, min(gamma, Hp) + 1):
        c = c * (Hp - g + 1) // g
        S += c
    return S


def state_masks(Hp, gamma):
    """The full state table as 16-bit masks (bit j = candidate position j), sizes 2..gamma, in the order of
    generate_state_matrix (by size, then lexicographic)."""
    out = []
    for g in range(2, min(gamma, Hp) + 1):
        for pos in itertools.combinations(range(Hp), g):
            out.append(sum(1 << p for p in pos))
    return np.asarray(out, dtype=np.uint16)


def mask_positions(mask):
    return tuple(j for j in range(16) if (int(mask) >> j) & 1)


def stats_len(H):
    return 2 * H * H + 3 * H + (XCD_COPIES - 1) * 2 * H * H


def stats_base(H):
    return 2 * H * H + 3 * H


# ------------------------------------------------------------------------------------------------------------ tables
def make_tables(Gd, psid, mu, pi, s2):
    """The eight rows the way GSC._tables_for builds them (float64 arithmetic), plus the ninth row [1 / s2, 0, 0, ...]."""
    Gd, psid, mu, pi = (np.asarray(x, dtype=np.float64) for x in (Gd, psid, mu, pi))
    lam = Gd / s2 + 1. / psid
    c0 = -(np.log(psid) + np.log(lam)) - mu * mu * Gd / s2
    lpi = np.log(pi) - np.log(1 - pi)
    t = np.zeros((9, len(Gd)))
    t[:8] = np.stack([c0, 2. * mu / s2, Gd * mu, 1. / (lam * s2 * s2), 1. / (lam * s2), 1. / lam, mu, lpi])
    t[8, 0] = 1.0 / s2
    return t


def with_thresholds(tables, thr=0.0, thr_p=0.0):
    """tables[8 H + 1] = thr (LIST), tables[8 H + 2] = thr_p; needs H >= 3."""
    t = np.array(tables, dtype=np.float64)
    H = t.shape[1]
    assert H >= 3
    t.reshape(-1)[8 * H + 1] = thr
    t.reshape(-1)[8 * H + 2] = thr_p
    return t


def inv_s2_of(c):
    """1 / sigma_sq as the launcher forms it (float64 division), or the ninth row's first entry when sigma_sq == 0."""
    return np.float64(1.0) / np.float64(c["sigma_sq"]) if c["sigma_sq"] > 0 else np.float64(c["tables"][8, 0])


# ---------------------------------------------------------------------------------------------------------- selection
def component_scores(c, rows=None, clamp=True):
    sl = slice(None) if rows is None else rows
    t = c["tables"].astype(LD)
    a, yn, inv = c["scores"][sl].astype(LD), c["ynorm2"][sl].astype(LD), LD(inv_s2_of(c))
    with np.errstate(invalid="ignore", over="ignore"):
        bb = a - t[2][None, :]
        v = (t[0][None, :] - yn[:, None] * inv + t[1][None, :] * a + bb * bb * t[3][None, :]).astype(np.float64)
        # the kernel's arithmetic is float64: where a product or the sum overflows there (+-inf, and NaN from inf - inf) the
        # float64 evaluation IS the result (any association gives the same non-finite value for the cases' inputs)
        t6, a6, yn6 = c["tables"], c["scores"][sl], c["ynorm2"][sl]
        b6 = a6 - t6[2][None, :]
        v6 = t6[0][None, :] - yn6[:, None] * np.float64(inv) + t6[1][None, :] * a6 + b6 * b6 * t6[3][None, :]
        v = np.where(np.isfinite(v6), v, v6)
        if clamp:
            v = np.where(np.isnan(v) | (v < -DBL_MAX), -DBL_MAX, v)
            v = np.where(np.isinf(v), 0.0, v)
    return v


def rank_values(v):
    """float64 scores with the low 10 mantissa bits dropped."""
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64) & ~np.uint64(0x3FF)
    return b.view(np.float64)


def select(c, rows=None):
    """(n, H') candidates: the H' largest ranking values, ties towards the larger index, sorted by index."""
    r = rank_values(component_scores(c, rows))
    H, Hp = r.shape[1], c["Hp"]
    out = np.zeros((r.shape[0], Hp), dtype=np.int32)
    for n in range(r.shape[0]):
        # -0.0 ranks below +0.0 (the keys are compared as sign-magnitude patterns): rank on (value, sign bit clear, index)
        order = sorted(range(H), key=lambda h: (r[n, h], not np.signbit(r[n, h]), h))
        out[n] = sorted(order[H - Hp:])
    return out


def selection_gap(c, rows=None):
    """Per row: |H'-th - (H'+1)-th largest score| / max(|both|) (inf where H' == H)."""
    v = np.sort(component_scores(c, rows), axis=1)
    Hp, H = c["Hp"], v.shape[1]
    if Hp == H:
        return np.full(v.shape[0], np.inf)
    a, b = v[:, H - Hp], v[:, H - Hp - 1]
    return np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), TINY)


# ------------------------------------------------------------------------------------------------------- g x g algebra
def gj_inverse(M):
    """Inverse and log|det| of (n, g, g) longdouble matrices: Gauss-Jordan without pivoting, as the kernel's."""
    M = np.array(M, dtype=LD)
    n, g, _ = M.shape
    ld = np.zeros(n, dtype=LD)
    for p in range(g):
        piv = M[:, p, p].copy()
        ld += np.log(np.abs(piv))
        ip = 1 / piv
        M[:, p, :] *= ip[:, None]
        M[:, p, p] = ip
        for r in range(g):
            if r == p:
                continue
            f = M[:, r, p].copy()
            M[:, r, :] -= f[:, None] * M[:, p, :]
            M[:, r, p] = -f * ip
    return M, ld


def state_terms(c, cand, pos, rows=None):
    """For the multi-cause state over candidate positions `pos`: lp (with the prior), kappa (n, g), Lambda^-1 (n, g, g),
    the cancellation term, and Psi_a, Lambda_a (for the conditioning cap)."""
    sl = slice(None) if rows is None else rows
    t = c["tables"].astype(LD)
    inv = LD(inv_s2_of(c))
    idx = cand[:, list(pos)]
    n = idx.shape[0]
    G = c["gram"].astype(LD)[idx[:, :, None], idx[:, None, :]]
    P = c["psi_sq"].astype(LD)[idx[:, :, None], idx[:, None, :]]
    a = np.take_along_axis(c["scores"][sl].astype(LD), idx, axis=1)
    yn = c["ynorm2"][sl].astype(LD)
    mu, prior = t[6][idx], t[7][idx].sum(axis=1)
    Pinv, ld1 = gj_inverse(P)
    Lam = Pinv + G * inv
    Linv, ld2 = gj_inverse(Lam)
    gmu = np.einsum("nij,nj->ni", G, mu)
    b = a - gmu
    r2 = yn + (mu * (gmu - 2 * a)).sum(axis=1)
    lb = np.einsum("nij,nj->ni", Linv, b)
    quad = (b * lb).sum(axis=1)
    kappa = lb * inv + mu
    lp = -(ld1 + ld2) - r2 * inv + quad * inv * inv + prior
    canc = U * (np.abs(yn) + (np.abs(mu) * (np.abs(gmu) + 2 * np.abs(a))).sum(axis=1)) * inv \
        + U * np.einsum("ni,nij,nj->n", np.abs(b), np.abs(Linv), np.abs(b)) * inv * inv
    return lp, kappa, Linv, canc, P, Lam


def weight(x):
    """exp(x) with the reference's clamp: NaN and everything below `tiny` -> tiny."""
    with np.errstate(under="ignore", invalid="ignore"):
        p = np.exp(np.asarray(x, dtype=LD))
    return np.where(np.isnan(p) | (p < LD(TINY)), LD(TINY), p)


def estep(c, cand, rows=None):
    """Everything a datapoint's pass computes, for the datapoints `rows` (all by default) with candidates `cand` (n, H')."""
    sl = slice(None) if rows is None else rows
    H, Hp, S, beta = c["H"], c["Hp"], c["S"], LD(c["beta"])
    t = c["tables"].astype(LD)
    inv = LD(inv_s2_of(c))
    a, yn = c["scores"][sl].astype(LD), c["ynorm2"][sl].astype(LD)
    n = a.shape[0]
    cand = np.asarray(cand, dtype=np.int64)
    K = 1 + H + S
    lp = np.zeros((n, K), dtype=LD)
    canc = np.zeros((n, K), dtype=LD)
    lp[:, 0] = -yn * inv
    canc[:, 0] = U * np.abs(yn) * inv
    bb = a - t[2][None, :]
    lp[:, 1:1 + H] = t[0][None, :] - yn[:, None] * inv + t[1][None, :] * a + bb * bb * t[3][None, :] + t[7][None, :]
    canc[:, 1:1 + H] = U * (np.abs(t[0])[None, :] + np.abs(yn)[:, None] * inv + np.abs(t[1][None, :] * a)
                            + bb * bb * np.abs(t[3])[None, :] + np.abs(t[7])[None, :])
    kap1 = bb * t[4][None, :] + t[6][None, :]
    w = np.zeros((n, K), dtype=LD)
    with np.errstate(under="ignore"):
        w[:, 0] = np.exp(beta * lp[:, 0])                                   # null state: not clamped
    w[:, 1:1 + H] = weight(beta * lp[:, 1:1 + H])
    ass = np.zeros((n, Hp, Hp), dtype=LD)
    aszsz = np.zeros((n, Hp, Hp), dtype=LD)
    as_ = np.zeros((n, Hp), dtype=LD)
    asz = np.zeros((n, Hp), dtype=LD)
    asz_abs = np.zeros((n, Hp), dtype=LD)
    for s in range(S):
        pos = mask_positions(c["masks"][s])
        l, kappa, Linv, cc, _, _ = state_terms(c, cand, pos, rows)
        lp[:, 1 + H + s], canc[:, 1 + H + s] = l, cc
        p = weight(beta * l)
        w[:, 1 + H + s] = p
        pl = list(pos)
        as_[:, pl] += p[:, None]
        asz[:, pl] += p[:, None] * kappa
        asz_abs[:, pl] += p[:, None] * np.abs(kappa)
        ix = np.ix_(range(n), pl, pl)
        ass[ix] += p[:, None, None]
        aszsz[ix] += p[:, None, None] * (kappa[:, :, None] * kappa[:, None, :] + Linv)
    Z = w.sum(axis=1)
    nf = 1 / (Z + LD(TINY))
    xs = w[:, 1:1 + H].copy()
    xsz = w[:, 1:1 + H] * kap1
    xsz_abs = np.abs(xsz)
    np.add.at(xs, (np.arange(n)[:, None], cand), as_)
    np.add.at(xsz, (np.arange(n)[:, None], cand), asz)
    np.add.at(xsz_abs, (np.arange(n)[:, None], cand), asz_abs)
    HH = Hp * Hp
    blocks = np.concatenate([ass.reshape(n, HH), aszsz.reshape(n, HH), as_, asz, w[:, 1 + H:].sum(axis=1)[:, None]], axis=1)
    return dict(lp=lp, canc=canc, w=w, Z=Z, nf=nf, xpt_s=xs * nf[:, None], xpt_sz=xsz * nf[:, None], blocks=blocks, xsz_abs=xsz_abs * nf[:, None],
                pair_ss=ass * nf[:, None, None], pair_zz=aszsz * nf[:, None, None],
                single_zz=w[:, 1:1 + H] * (kap1 * kap1 + t[5][None, :]) * nf[:, None], cand=cand)


# ---------------------------------------------------------------------------------------------------------- statistics
def raw_stats(c, e, lacc, thr_p=0.0, mult=None):
    """What a call adds to [U_ss | U_zz | cs | csz | dzz] (stats_base(H) entries).  `lacc`: the diagonal of the pair blocks
    of xpt_szsz goes to dzz (and is always kept), else into U_zz.  thr_p: an entry of a datapoint's pair blocks is sent
    when vss > thr_p resp. |vzz| > thr_p; read only when sigma_sq == 0 and H > 2 (the caller passes 0 otherwise)."""
    H, Hp = c["H"], c["Hp"]
    n = e["xpt_s"].shape[0]
    m = np.ones(n, dtype=LD) if mult is None else np.asarray(mult, dtype=LD)
    HH = H * H
    add = np.zeros(stats_base(H), dtype=LD)
    U_ss, U_zz = add[:HH].reshape(H, H), add[HH:2 * HH].reshape(H, H)
    dzz = add[2 * HH + 2 * H:]
    cand = e["cand"]
    thr_p = LD(thr_p)
    for i in range(Hp):
        for k in range(Hp):
            vss, vzz = e["pair_ss"][:, i, k], e["pair_zz"][:, i, k]
            if k > i:
                np.add.at(U_ss, (cand[:, i], cand[:, k]), np.where(vss > thr_p, vss, 0) * m)
            if lacc and k == i:
                np.add.at(dzz, cand[:, i], vzz * m)
            else:
                np.add.at(U_zz, (cand[:, i], cand[:, k]), np.where(np.abs(vzz) > thr_p, vzz, 0) * m)
    add[2 * HH:2 * HH + H] = (e["xpt_s"] * m[:, None]).sum(axis=0)
    add[2 * HH + H:2 * HH + 2 * H] = (e["xpt_sz"] * m[:, None]).sum(axis=0)
    dzz += (e["single_zz"] * m[:, None]).sum(axis=0)
    return add


def packed_stats(raw, H, yy):
    """pm_gsc_pack_stats_f64 of a raw statistics buffer (any float type)."""
    HH = H * H
    U_ss, U_zz = raw[:HH].reshape(H, H), raw[HH:2 * HH].reshape(H, H)
    cs, csz, dzz = raw[2 * HH:2 * HH + H], raw[2 * HH + H:2 * HH + 2 * H], raw[2 * HH + 2 * H:2 * HH + 3 * H]
    up = np.triu(U_ss, 1)
    ss = up + up.T + np.diag(cs)
    zz = U_zz + np.diag(dzz)
    return np.concatenate([ss.reshape(-1), zz.reshape(-1), cs, csz, np.asarray([yy], dtype=raw.dtype)])


SECTIONS_RAW = ("U_ss", "U_zz", "cs", "csz", "dzz")
SECTIONS_PACKED = ("ss", "zz", "s", "sz", "yy")


def sections(H, packed=False):
    HH = H * H
    if packed:
        return dict(ss=slice(0, HH), zz=slice(HH, 2 * HH), s=slice(2 * HH, 2 * HH + H), sz=slice(2 * HH + H, 2 * HH + 2 * H),
                    yy=slice(2 * HH + 2 * H, 2 * HH + 2 * H + 1))
    return dict(U_ss=slice(0, HH), U_zz=slice(HH, 2 * HH), cs=slice(2 * HH, 2 * HH + H), csz=slice(2 * HH + H, 2 * HH + 2 * H),
                dzz=slice(2 * HH + 2 * H, 2 * HH + 3 * H))


# --------------------------------------------------------------------------------------------------------------- lists
def list_split(xs, xsz, thr):
    """LIST form: per row the entries with |xpt_sz| > thr or xpt_s > thr; at most 16 -> a list in latent order (nz_idx with
    0xFFFF behind the last entry, two value planes; -1 marks a value slot the kernel does not write), else an empty list
    and a dense row.  Returns (idx (n, 16) uint16, vz (n, 16), vs (n, 16), written (n, 16) bool, dense row indices)."""
    n, H = xs.shape
    idx = np.full((n, NZ_MAX), 0xFFFF, dtype=np.uint16)
    vz = np.zeros((n, NZ_MAX), dtype=LD)
    vs = np.zeros((n, NZ_MAX), dtype=LD)
    written = np.zeros((n, NZ_MAX), dtype=bool)
    dense = []
    thr = LD(thr)
    nsig = np.zeros(n, dtype=np.int64)
    for r in range(n):
        sig = np.nonzero((np.abs(xsz[r]) > thr) | (xs[r] > thr))[0]
        nsig[r] = len(sig)
        if len(sig) <= NZ_MAX:
            k = len(sig)
            idx[r, :k] = sig
            vz[r, :k], vs[r, :k] = xsz[r, sig], xs[r, sig]
            written[r, :k] = True
        else:
            dense.append(r)
    return idx, vz, vs, written, np.asarray(dense, dtype=np.int64), nsig


def list_pairs(idx, vs, vz, H):
    """[sum_n xs_n xsz_n^T | sum_n xsz_n xsz_n^T] (2 H H) over the listed entries; slots behind a terminator are not read."""
    out = np.zeros((2, H, H), dtype=LD)
    for r in range(idx.shape[0]):
        k = int(np.argmax(idx[r] == 0xFFFF)) if (idx[r] == 0xFFFF).any() else NZ_MAX
        ii = idx[r, :k].astype(np.int64)
        s, z = np.asarray(vs[r, :k], dtype=LD), np.asarray(vz[r, :k], dtype=LD)
        out[0][np.ix_(ii, ii)] += s[:, None] * z[None, :]
        out[1][np.ix_(ii, ii)] += z[:, None] * z[None, :]
    return out.reshape(-1)


# --------------------------------------------------------------------------------------------------------------- cases
# name: (H, H', gamma, S (None: the full table; else a prefix of it), N, flags, (VPL, GMAX, form), psi symmetric)
# One smallest shape per reachable (VPL, GMAX, form) cell of pm_gsc_plan(PM_GSC_PLAN_ESTEP); both ends of H of every VPL
# bucket appear.  N: 16 < N < 64, not a multiple of 16, unless stated.
CASES = {
    # ---- LACC (statistics form, the LDS accumulators fit)
    "a_v1_g2": (1, 1, 1, None, 19, 0, (1, 2, LACC), True),                 # H = 1, no multi-cause state
    "a_v1_g3": (16, 4, 3, None, 37, 0, (1, 3, LACC), False),
    "a_v1_g4": (13, 5, 4, None, 21, 0, (1, 4, LACC), True),
    "a_v1_g6": (16, 6, 5, None, 18, 0, (1, 6, LACC), False),
    "a_v1_g8": (9, 8, 8, None, 17, 0, (1, 8, LACC), True),
    "a_v2_g2": (17, 3, 2, None, 33, 0, (2, 2, LACC), False),
    "a_v2_g3": (32, 5, 3, None, 23, 0, (2, 3, LACC), True),
    "a_v2_g4": (20, 4, 4, None, 19, 0, (2, 4, LACC), False),
    "a_v2_g6": (31, 6, 6, None, 17, 0, (2, 6, LACC), True),
    "a_v2_g8": (17, 7, 7, None, 17, 0, (2, 8, LACC), False),
    "a_v4_g2": (33, 2, 2, None, 47, 0, (4, 2, LACC), True),
    "a_v4_g3": (64, 3, 3, None, 19, 0, (4, 3, LACC), False),
    "a_v4_g4": (40, 5, 4, None, 18, 0, (4, 4, LACC), True),
    "a_v4_g6": (33, 6, 5, None, 17, 0, (4, 6, LACC), False),
    "a_v4_g8": (64, 8, 7, None, 17, 0, (4, 8, LACC), True),
    "a_v8_g2": (65, 6, 2, None, 21, 0, (8, 2, LACC), False),
    "a_v8_g3": (128, 4, 3, None, 35, 0, (8, 3, LACC), True),
    "a_v8_g4": (100, 4, 4, None, 17, 0, (8, 4, LACC), False),
    "a_v8_g6": (65, 6, 6, None, 17, 0, (8, 6, LACC), True),
    "a_v8_g8": (128, 7, 7, None, 17, 0, (8, 8, LACC), False),
    "a_v16_g2": (129, 3, 2, None, 18, 0, (16, 2, LACC), True),
    "a_v16_g3": (256, 3, 3, None, 17, 0, (16, 3, LACC), False),
    "a_v16_g4": (200, 4, 4, None, 17, 0, (16, 4, LACC), True),
    "a_v16_g6": (129, 5, 5, None, 17, 0, (16, 6, LACC), False),
    "a_v16_g8": (256, 3, 7, None, 17, 0, (16, 8, LACC), True),
    # (VPL = 32 fits the LACC layout at H <= 297 and H' = 1 only: no multi-cause state, whatever gamma asks for)
    "a_v32_g2": (257, 1, 2, None, 18, 0, (32, 2, LACC), True),
    "a_v32_g3": (297, 1, 3, None, 17, 0, (32, 3, LACC), False),
    "a_v32_g4": (260, 1, 4, None, 17, 0, (32, 4, LACC), True),
    "a_v32_g6": (297, 1, 6, None, 17, 0, (32, 6, LACC), False),
    "a_v32_g8": (257, 1, 8, None, 17, 0, (32, 8, LACC), True),
    # ---- plain (the LACC layout exceeds 53 KB)
    "p_v1_g2": (10, 10, 2, None, 19, 0, (1, 2, PLAIN), False),
    "p_v1_g3": (16, 10, 3, None, 18, 0, (1, 3, PLAIN), True),
    "p_v1_g4": (12, 10, 4, None, 17, 0, (1, 4, PLAIN), False),
    "p_v1_g6": (16, 10, 5, None, 17, 0, (1, 6, PLAIN), True),
    "p_v1_g8": (11, 10, 7, None, 17, 0, (1, 8, PLAIN), False),
    "p_v2_g2": (17, 10, 2, None, 21, 0, (2, 2, PLAIN), True),
    "p_v2_g3": (32, 10, 3, None, 17, 0, (2, 3, PLAIN), False),
    "p_v2_g4": (24, 10, 4, None, 17, 0, (2, 4, PLAIN), True),
    "p_v2_g6": (32, 10, 6, None, 17, 0, (2, 6, PLAIN), False),
    "p_v2_g8": (17, 10, 8, None, 17, 0, (2, 8, PLAIN), True),
    "p_v4_g2": (33, 10, 2, None, 17, 0, (4, 2, PLAIN), False),
    "p_v4_g3": (64, 9, 3, None, 17, 0, (4, 3, PLAIN), True),
    "p_v4_g4": (48, 10, 4, None, 17, 0, (4, 4, PLAIN), False),
    "p_v4_g6": (64, 9, 6, None, 17, 0, (4, 6, PLAIN), True),
    "p_v4_g8": (33, 10, 8, None, 17, 0, (4, 8, PLAIN), False),
    "p_v8_g2": (65, 9, 2, None, 18, 0, (8, 2, PLAIN), True),
    "p_v8_g3": (128, 8, 3, None, 17, 0, (8, 3, PLAIN), False),
    "p_v8_g4": (96, 9, 4, None, 17, 0, (8, 4, PLAIN), True),
    "p_v8_g6": (128, 8, 5, None, 17, 0, (8, 6, PLAIN), False),
    "p_v8_g8": (65, 9, 8, None, 17, 0, (8, 8, PLAIN), True),
    "p_v16_g2": (129, 8, 2, None, 17, 0, (16, 2, PLAIN), False),
    "p_v16_g3": (256, 5, 3, None, 19, 0, (16, 3, PLAIN), True),
    "p_v16_g4": (180, 7, 4, None, 17, 0, (16, 4, PLAIN), False),
    "p_v16_g6": (256, 5, 5, None, 17, 0, (16, 6, PLAIN), True),
    "p_v16_g8": (129, 8, 8, None, 17, 0, (16, 8, PLAIN), False),
    "p_v32_g2": (257, 5, 2, None, 18, 0, (32, 2, PLAIN), True),
    "p_v32_g3": (512, 3, 3, None, 17, 0, (32, 3, PLAIN), False),
    "p_v32_g4": (300, 4, 4, None, 17, 0, (32, 4, PLAIN), True),
    "p_v32_g6": (257, 6, 6, None, 17, 0, (32, 6, PLAIN), False),
    "p_v32_g8": (512, 7, 7, None, 17, 0, (32, 8, PLAIN), True),
    # ---- LPJ (log-joints written; statistics as the plain form; `p`: on the plain LDS layout)
    "l_v1_g2p": (16, 10, 2, None, 19, F_LPJ, (1, 2, LPJ), True),
    "l_v1_g3": (7, 4, 3, None, 21, F_LPJ, (1, 3, LPJ), False),
    "l_v1_g4": (16, 4, 4, None, 17, F_LPJ, (1, 4, LPJ), True),
    "l_v1_g6": (8, 5, 5, None, 17, F_LPJ, (1, 6, LPJ), False),
    "l_v1_g8": (16, 7, 7, None, 17, F_LPJ, (1, 8, LPJ), True),
    "l_v2_g2": (17, 2, 2, None, 18, F_LPJ, (2, 2, LPJ), False),
    "l_v2_g3": (32, 3, 3, None, 17, F_LPJ, (2, 3, LPJ), True),
    "l_v2_g4": (32, 4, 4, None, 17, F_LPJ, (2, 4, LPJ), False),
    "l_v2_g6": (17, 6, 6, None, 17, F_LPJ, (2, 6, LPJ), True),
    "l_v2_g8p": (20, 10, 7, None, 17, F_LPJ, (2, 8, LPJ), False),
    "l_v4_g2": (33, 5, 2, None, 18, F_LPJ, (4, 2, LPJ), True),
    "l_v4_g3p": (64, 9, 3, None, 17, F_LPJ, (4, 3, LPJ), False),
    "l_v4_g4": (33, 4, 4, None, 17, F_LPJ, (4, 4, LPJ), True),
    "l_v4_g6": (64, 5, 5, None, 17, F_LPJ, (4, 6, LPJ), False),
    "l_v4_g8": (50, 8, 8, None, 17, F_LPJ, (4, 8, LPJ), True),
    "l_v8_g2": (128, 3, 2, None, 17, F_LPJ, (8, 2, LPJ), False),
    "l_v8_g3": (65, 4, 3, None, 17, F_LPJ, (8, 3, LPJ), True),
    "l_v8_g4p": (128, 8, 4, None, 17, F_LPJ, (8, 4, LPJ), False),
    "l_v8_g6": (65, 5, 5, None, 17, F_LPJ, (8, 6, LPJ), True),
    "l_v8_g8": (100, 7, 8, None, 17, F_LPJ, (8, 8, LPJ), False),
    "l_v16_g2": (256, 2, 2, None, 17, F_LPJ, (16, 2, LPJ), True),
    "l_v16_g3p": (129, 8, 3, None, 17, F_LPJ, (16, 3, LPJ), False),
    "l_v16_g4": (129, 4, 4, None, 17, F_LPJ, (16, 4, LPJ), True),
    "l_v16_g6p": (256, 6, 6, None, 17, F_LPJ, (16, 6, LPJ), False),
    "l_v16_g8p": (129, 7, 7, None, 17, F_LPJ, (16, 8, LPJ), True),
    "l_v32_g2p": (512, 4, 2, None, 17, F_LPJ, (32, 2, LPJ), False),
    "l_v32_g3p": (257, 3, 3, None, 17, F_LPJ, (32, 3, LPJ), True),
    "l_v32_g4p": (257, 5, 4, None, 17, F_LPJ, (32, 4, LPJ), False),
    "l_v32_g6p": (512, 6, 6, None, 17, F_LPJ, (32, 6, LPJ), True),
    "l_v32_g8p": (300, 7, 7, None, 17, F_LPJ, (32, 8, LPJ), False),
    # ---- LIST
    "t_v8_g2": (65, 4, 2, None, 37, F_LISTS, (8, 2, LIST), False),
    "t_v8_g3": (128, 4, 3, None, 21, F_LISTS, (8, 3, LIST), True),
    "t_v16_g2": (129, 3, 2, None, 19, F_LISTS, (16, 2, LIST), False),
    "t_v16_g3": (256, 3, 3, None, 18, F_LISTS, (16, 3, LIST), True),
}
# state-trip edges: S in {0, 1, 15, 16, 17} (a prefix of the full table of H' = 6, gamma = 3: 35 states, where no table of
# that size exists); `e_s0_hp1`: gamma = 1 and H' = 1
EDGE_CASES = {
    "e_s0_g1": (8, 3, 1, None, 19, 0, (1, 2, LACC), True),
    "e_s0_hp1": (20, 1, 3, None, 17, 0, (2, 3, LACC), False),
    "e_s1": (8, 2, 2, None, 17, 0, (1, 2, LACC), True),
    "e_s15": (12, 6, 2, None, 18, 0, (1, 2, LACC), False),
    "e_s16": (12, 6, 3, 16, 17, 0, (1, 3, LACC), True),
    "e_s17": (12, 6, 3, 17, 21, 0, (1, 3, LACC), False),
}
THRESHOLD_CASES = ("a_v1_g3", "p_v2_g2", "a_v8_g3", "l_v4_g2")
H2_CASE = "h2"
CASES_EXTRA = {H2_CASE: (2, 2, 2, None, 19, 0, (1, 2, LACC), False)}
ALL_CASES = dict(CASES, **EDGE_CASES, **CASES_EXTRA)
# the refusals of pm_gsc_plan: (which, H, H', S (None: full), gamma, D, flags, N) -> return code
EINVAL, ERANGE = -1, -2
REFUSALS = [
    ((ESTEP, 0, 1, 0, 1, 0, 0, 16), EINVAL), ((ESTEP, 8, 0, 0, 1, 0, 0, 16), EINVAL), ((ESTEP, 8, 2, -1, 2, 0, 0, 16), EINVAL),
    ((ESTEP, 8, 2, None, 2, 0, 0, 0), EINVAL), ((ESTEP, 8, 2, None, 2, 0, 8, 16), EINVAL),
    ((ESTEP, 8, 2, None, 2, 0, F_BLOCKS, 16), EINVAL), ((ESTEP, 128, 2, None, 2, 0, F_LISTS | F_LPJ, 16), EINVAL),
    ((4, 8, 2, None, 2, 0, 0, 16), EINVAL), ((-1, 8, 2, None, 2, 0, 0, 16), EINVAL),
    ((ESTEP, 513, 2, None, 2, 0, 0, 16), ERANGE), ((ESTEP, 8, 9, None, 2, 0, 0, 16), ERANGE),
    ((ESTEP, 32, 17, None, 2, 0, 0, 16), ERANGE), ((ESTEP, 8, 2, None, 0, 0, 0, 16), ERANGE),
    ((ESTEP, 8, 2, None, 9, 0, 0, 16), ERANGE),
    ((ESTEP, 129, 10, None, 2, 0, 0, 16), ERANGE),                          # the full table's layout exceeds 64 KB
    ((ESTEP, 16, 10, 5000, 2, 0, 0, 16), ERANGE),                           # ... and so does this table handed in
    ((ESTEP, 64, 4, None, 2, 0, F_LISTS, 16), ERANGE), ((ESTEP, 257, 3, None, 2, 0, F_LISTS, 16), ERANGE),
    ((ESTEP, 128, 4, None, 4, 0, F_LISTS, 16), ERANGE), ((ESTEP, 128, 9, None, 2, 0, F_LISTS, 16), ERANGE),   # gamma; !lacc
    ((ESTEP, 128, 4, None, 2, 100, F_LISTS, 16), ERANGE), ((ESTEP, 192, 4, None, 2, 128, F_LISTS, 16), ERANGE),   # D
    ((LIST_PAIRS, 320, 0, 0, 0, 0, 0, 16), ERANGE), ((LIST_PAIRS, 100, 0, 0, 0, 0, 0, 16), ERANGE),
    ((LIST_PAIRS, 0, 0, 0, 0, 0, 0, 16), EINVAL), ((LIST_PAIRS, 64, 0, 0, 0, 0, 0, 0), EINVAL),
    ((PACK, 513, 0, 0, 0, 0, 0, 1), ERANGE), ((PACK, 0, 0, 0, 0, 0, 0, 1), EINVAL),
    ((COMPONENT_SCORES, 512, 0, 0, 0, 0, 0, 1 << 41), ERANGE), ((COMPONENT_SCORES, 0, 0, 0, 0, 0, 0, 5), EINVAL),
]
# list pairs: H -> (rows_c, nchunks, datapoint groups at N = 45, rows per group)
LIST_PAIRS_CELLS = {64: (64, 1, 1, 64), 128: (128, 1, 1, 64), 192: (64, 3, 1, 64), 256: (64, 4, 1, 64)}


def case_shape(name):
    H, Hp, gamma, S, N, flags, cell, sym = ALL_CASES[name]
    return dict(name=name, H=H, Hp=Hp, gamma=gamma, S=full_states(Hp, gamma) if S is None else S, N=N, flags=flags, cell=cell,
                sym=sym)


def make_case(name, hot, N=None, seed=0):
    """Operands of a case, built directly as kernel inputs.  HOT: W small, sigma_sq large, pi = 1/2, psi_sq near I,
    beta = 1.5.  COLD: sigma_sq = 1, beta = 1.25, |y|^2 set per row so that beta lp of the row's states lies around
    log(tiny): rows cycle through [all states far above (around -600) | the median state at -708.2, inside the libm window | every state,
    the null state included, below log(tiny) | the median state just below log(tiny)]."""
    c = case_shape(name)
    H, Hp, gamma, S = c["H"], c["Hp"], c["gamma"], c["S"]
    N = c["N"] if N is None else N
    c["N"] = N
    rng = np.random.RandomState(1000 * H + 10 * Hp + gamma + (7 if hot else 0) + seed)
    c["hot"] = hot
    c["masks"] = state_masks(Hp, gamma)[:S]
    assert len(c["masks"]) == S
    wscale, s2, beta = (0.1, 48.0, 1.5) if hot else (1.0, 1.0, 1.25)
    # gram: symmetric, diagonally dominant inside every H' x H' block; psi_sq: near I, non-symmetric unless `sym`
    off = rng.uniform(-1, 1, size=(H, H))
    gram = wscale ** 2 * (np.diag(rng.uniform(0.8, 1.3, size=H)) + 0.04 * (off + off.T) * (1 - np.eye(H)))
    psi = np.diag(rng.uniform(0.8, 1.3, size=H)) + 0.05 * rng.uniform(-1, 1, size=(H, H)) * (1 - np.eye(H))
    if c["sym"]:
        psi = 0.5 * (psi + psi.T)
    mu = rng.uniform(-0.5, 0.5, size=H)
    pi = np.full(H, 0.5) if hot else rng.uniform(0.2, 0.6, size=H)
    c["gram"], c["psi_sq"] = gram, psi
    c["tables"] = make_tables(np.diag(gram).copy(), np.diag(psi).copy(), mu, pi, s2)
    c["sigma_sq"], c["beta"] = s2, beta
    c["scores"] = wscale * rng.uniform(-1.5, 1.5, size=(N, H))
    c["ynorm2"] = rng.uniform(0.5, 4.0, size=N)
    if not hot:
        # lp of every state is linear in |y|^2 with slope -1 / s2: place each row's states around log(tiny)
        base = dict(c, ynorm2=np.zeros(N))
        cand = select(base)
        lp0 = np.asarray(estep(base, cand)["lp"], dtype=np.float64)
        med, top = np.sort(lp0[:, 1:], axis=1)[:, (lp0.shape[1] - 1) // 2], lp0.max(axis=1)      # (a non-null state)
        kind = np.arange(N) % 4
        target = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [-600.0, -708.2, -712.0, -708.5])
        anchor = np.where(kind == 2, top, med)
        c["ynorm2"] = (anchor - target / beta) * s2
        assert (c["ynorm2"] > 0).all()
    return c


# ----------------------------------------------------------------------------------------------------- selection cases
def make_selection_case(H, Hp, seed=0):
    """Exact scores: integer scores and |y|^2, sigma_sq = 4, dyadic c0, c1, gm, il -- every product and partial sum of
    c0 - yn / s2 + c1 a + (a - gm)^2 il is a dyadic rational of a few bits, so any evaluation order (fused or not) gives the
    same float64.  Rows: [0, 8) random integers with ties at the cut and inside the selected set; then all +0.0; a row whose
    clamps give 0 (from +inf, beating negative scores and losing to positive ones); a row with NaN scores (-> -DBL_MAX)
    beside finite ones; |y|^2 = +inf (every score -inf -> -DBL_MAX); |y|^2 = NaN."""
    rng = np.random.RandomState(77 * H + Hp + seed)
    N = 13
    c = dict(name="sel_%d_%d" % (H, Hp), H=H, Hp=Hp, gamma=1, S=0, N=N, flags=0, hot=True, sigma_sq=4.0, beta=1.0)
    t = np.zeros((9, H))
    t[0] = rng.randint(0, 2, size=H) / 2.0                # c0
    t[1] = 2.0                                            # c1
    t[2] = rng.randint(0, 2, size=H).astype(np.float64)   # gm
    t[3] = 0.25                                           # il
    t[4], t[5], t[6], t[7] = 0.5, 1.0, 0.0, 0.0
    t[8, 0] = 0.25
    a = rng.randint(-6, 7, size=(N, H)).astype(np.float64)
    yn = rng.randint(0, 9, size=N).astype(np.float64)
    # rows 0..3: few distinct values -> many ties; row 4: every score equal
    a[:4] = rng.randint(-1, 2, size=(4, H))
    t0 = t.copy()
    a[8], yn[8] = 0.0, 0.0
    a[9], yn[9] = -3.0, 40.0                              # all negative ...
    a[9, rng.permutation(H)[:max(1, min(H - 1, Hp // 2))]] = 1e308          # ... but these: c1 a = +inf -> 0
    if H > 2:
        a[9, (int(np.argmax(a[9] == 1e308)) + 1) % H] = 30.0                # and one large finite positive score
    a[10] = rng.randint(-6, 7, size=H)
    a[10, rng.permutation(H)[:max(1, H // 3)]] = -1e308   # c1 a = -inf, (a - gm)^2 il = +inf: NaN -> -DBL_MAX
    yn[11], yn[12] = np.inf, np.nan
    c["tables"], c["scores"], c["ynorm2"] = t0, a, yn
    c["gram"] = np.eye(H)
    c["psi_sq"] = np.eye(H)
    c["masks"] = np.zeros(0, dtype=np.uint16)
    return c


def make_zero_case(H, Hp, negative):
    """Every score exactly +0.0 (c0 = gm = 0, a = 0, |y|^2 = 0) or -0.0 (c0 = -0.0, c1 = -1 on a = +0.0, il = -0.0): the keys
    are subnormals that differ in the index bits alone."""
    c = make_selection_case(H, Hp)
    t = np.zeros((9, H))
    t[1], t[3], t[4], t[5] = 0.5, 0.25, 0.5, 1.0
    if negative:
        t[0], t[1], t[3] = -0.0, -1.0, -0.0
    t[8, 0] = 0.25
    c["tables"] = t
    c["N"] = 3
    c["scores"], c["ynorm2"] = np.zeros((3, H)), np.zeros(3)
    c["name"] = "zero_%s_%d_%d" % ("neg" if negative else "pos", H, Hp)
    return c


# ---------------------------------------------------------------------------------------------------------- thresholds
def clear_of(thr, values):
    """No value lies within a factor 1 +- 2^-20 of thr."""
    v = np.abs(np.asarray(values, dtype=LD).reshape(-1))
    return thr == 0 or bool((np.abs(v / LD(thr) - 1) > LD(2.0) ** -20).all())


def pair_values(e):
    """Every value the thr_p rule looks at: the strict upper triangle of a datapoint's xpt_ss block and all of |xpt_szsz|."""
    Hp = e["pair_ss"].shape[1]
    iu = np.triu_indices(Hp, 1)
    return np.concatenate([e["pair_ss"][:, iu[0], iu[1]].reshape(-1), np.abs(e["pair_zz"]).reshape(-1)])


def pick_thr_p(e):
    """A thr_p that drops some entries and keeps others: the middle of the widest relative gap in the second and third
    quarter of the sorted values."""
    v = np.sort(pair_values(e))
    v = v[v > 0]
    lo, hi = len(v) // 4, 3 * len(v) // 4
    k = lo + int(np.argmax(v[lo + 1:hi + 1] / v[lo:hi]))
    return float(np.sqrt(v[k] * v[k + 1]))


def list_measure(xs, xsz):
    """A row's entry is significant when max(|xpt_sz|, xpt_s) > thr."""
    return np.maximum(np.abs(xsz), xs)


def thr_for_count(xs, xsz, k):
    """(row, thr): a thr that leaves `row` exactly k significant entries (k = 0: none) and is clear of every value of every
    row; the first row that allows it."""
    m = list_measure(xs, xsz)
    for row in range(m.shape[0]):
        r = np.sort(m[row])[::-1]
        thr = float(r[0] * 2) if k == 0 else float(np.sqrt(r[k - 1] * r[k]))
        if clear_of(thr, m) and (k == 0 or r[k - 1] > thr > r[k]):
            return row, thr
    raise AssertionError("no row leaves room for a threshold with %d entries above it" % k)
