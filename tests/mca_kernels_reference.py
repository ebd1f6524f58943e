"""Plain NumPy reference (np.longdouble) of the MCA / MMCA kernels (mca_kernels.hip) as include/prosper_hip.h states them and
oracle/mca_oracle.py / oracle/mmca_oracle.py restate them, operand for operand as the C ABI takes them: scores = Y W^T,
wnorm2, ynorm2, Wrho = sign(W)|W|^rho, Wrm1 = |W|^(rho-1) are float64 INPUTS of the kernels, so the reference starts from the
same float64 tables and carries everything behind them in longdouble.

  select_scores    R[n,h] = sum_d max(W_hd - y_d, 0)
  logpj            [pre1 |y|^2 | pil_bar + pre1 (|W_h|^2 - 2 <W_h, y> + |y|^2) (the Gram identity) |
                    pil_bar |s| + pre1 sum_d (Wbar_sd - y_d)^2,  Wbar = sign(t)|t|^(1/rho),  t = sum_{j in s} Wrho[c_j, d]]
  lse              lse1 = log sum_k exp(f_k), lseb = log sum_k exp(beta f_k)
  aid_blocks       Aid[n,j,d] = sum_{s: j in s} q_s fac_sjd,  q_s = exp(beta f_s - lseb);  unsigned W: fac = t^(1/rho - 1)
                   Wrm1[c_j, d];  signed W: fac = min(1, |t|^(1/rho - 1) Wrm1[c_j, d]), and 1 where t = 0
  packed_stats     [G1 (not touched) | Wp_m | Wq_m | q1sum | sum q |s|, sum q e, sum lse1, count] over a keep mask
  defer_records    the Aid blocks and [sum q |s|, sum q e, lse1, 0] per datapoint
  defer_apply      what pm_mca_defer_apply_f64 adds from records, scalars and q1 over the kept set
  w_update         (G1 W^2 + Wp_m) / (q1sum W^2 + Wq_m), 0 / tiny below the smallest normal

Drop rules, the documented ones and no others: a weight that underflows to exactly 0 in float64 adds nothing (exp of less than
UNDERFLOW); the log-evidence sums leave out terms with f_k - max f <= -745 (the |s| = 0 term aside); the two-pass M-step
(`qcut`) leaves out multi-cause states with beta f_s - lseb <= -745.2.

CASES and make_case(name, hot) hold one smallest shape per dispatch cell for guarded-operand tests through the C ABI;
tests/test_mca_kernels_cpu.py pins this file against the oracles and asserts what such a test relies on for every case."""
import itertools

import numpy as np

LD = np.longdouble
UNDERFLOW = -745.1332191019412        # exp(x) rounds to 0 in float64 below this (half the smallest subnormal)
LSE_CUT = -745.0
QCUT = -745.2
NSCALARS = 4
ESTEP, MSTEP_ROWS, FUSED, DEFER_APPLY = 0, 1, 2, 3      # PM_MCA_PLAN_*
PLAN_LEN = 16
TINY = 2.2250738585072014e-308


def rho_of(T, bound):
    return 1.0 / (1.0 - 1.0 / max(T, bound))


# ---------------------------------------------------------------------------------------------------------- selection
def select_scores(Y, W):
    Y, W = np.asarray(Y, dtype=LD), np.asarray(W, dtype=LD)
    return np.maximum(W[None, :, :] - Y[:, None, :], 0).sum(axis=2)


# -------------------------------------------------------------------------------------------------------------- tables
def tables(W, rho, signed):
    """float64 Wrho, Wrm1, wnorm2 of W (H, D), rounded once from longdouble."""
    Wl = np.asarray(W, dtype=LD)
    a = np.abs(Wl)
    with np.errstate(divide="ignore"):
        wrho = np.where(a > 0, np.sign(Wl) * np.exp(LD(rho) * np.log(np.where(a > 0, a, 1))), 0)
        wrm1 = np.where(a > 0, np.exp(LD(rho - 1.0) * np.log(np.where(a > 0, a, 1))), 0)
    return wrho.astype(np.float64), wrm1.astype(np.float64), (Wl * Wl).sum(axis=1).astype(np.float64)


def state_bits(masks, Hp):
    """(S, Hp) 0/1 matrix of the 16-bit state masks (bit j = candidate position j)."""
    m = np.asarray(masks, dtype=np.int64)
    return ((m[:, None] >> np.arange(Hp)[None, :]) & 1).astype(np.int64)


def _tsum(c, rows=None):
    """t[n, s, d] = sum of the state's Wrho rows, in longdouble (the inputs are float64)."""
    SM = state_bits(c["masks"], c["Hp"]).astype(LD)
    cand = c["cand"] if rows is None else c["cand"][rows]
    return np.einsum("sj,njd->nsd", SM, c["Wrho"].astype(LD)[cand])


# ---------------------------------------------------------------------------------------------------------- log-joints
def logpj(c, rows=None):
    """(n, 1 + H + S) log-pseudo-joints of the datapoints `rows` (all by default), longdouble."""
    sl = slice(None) if rows is None else rows
    Y = c["Y"][sl].astype(LD)
    yn = c["ynorm2"][sl].astype(LD)
    pil, pre1 = LD(c["pil_bar"]), LD(c["pre1"])
    e1 = c["wnorm2"].astype(LD)[None, :] - 2 * c["scores"][sl].astype(LD) + yn[:, None]
    out = [pre1 * yn[:, None], pil + pre1 * e1]
    if c["S"]:
        t = _tsum(c, rows)
        a = np.abs(t)
        with np.errstate(divide="ignore"):
            wbar = np.where(a > 0, np.sign(t) * np.exp(np.log(np.where(a > 0, a, 1)) * LD(c["inv_rho"])), 0)
        es = ((wbar - Y[:, None, :]) ** 2).sum(axis=2)
        ns = state_bits(c["masks"], c["Hp"]).sum(axis=1).astype(LD)
        out.append(pil * ns[None, :] + pre1 * es)
    return np.concatenate(out, axis=1)


def lse(F, beta):
    """(lse1, lseb); terms at or below LSE_CUT of the row maximum are left out of both sums (never the first)."""
    F = np.asarray(F, dtype=LD)
    m = F.max(axis=1)
    dl = F - m[:, None]
    use = dl > LSE_CUT
    use[:, 0] = True
    s1 = np.where(use, np.exp(dl), 0).sum(axis=1)
    sb = np.where(use, np.exp(LD(beta) * dl), 0).sum(axis=1)
    return m + np.log(s1), LD(beta) * m + np.log(sb)


def posteriors(c, F, lseb, qcut=None):
    """q (n, 1 + H + S) = exp(beta f - lseb), 0 where float64 underflows (and, given qcut, for multi-cause states at or
    below it)."""
    dl = LD(c["beta"]) * np.asarray(F, dtype=LD) - np.asarray(lseb, dtype=LD)[:, None]
    q = np.where(dl >= UNDERFLOW, np.exp(dl), 0)
    if qcut is not None:
        q[:, 1 + c["H"]:] = np.where(dl[:, 1 + c["H"]:] > qcut, q[:, 1 + c["H"]:], 0)
    return q


# ----------------------------------------------------------------------------------------------------------- Aid block
def aid_blocks(c, qs, rows=None):
    """Aid (n, Hp, D) from the multi-cause posteriors qs (n, S)."""
    n = qs.shape[0]
    if not c["S"]:
        return np.zeros((n, c["Hp"], c["D"]), dtype=LD)
    cand = c["cand"] if rows is None else c["cand"][rows]
    SM = state_bits(c["masks"], c["Hp"]).astype(LD)
    t = _tsum(c, rows)
    a = np.abs(t)
    with np.errstate(divide="ignore"):
        r = np.where(a > 0, np.exp(np.log(np.where(a > 0, a, 1)) * LD(c["inv_rho"] - 1.0)), np.inf)     # |t|^(1/rho - 1)
    wm = c["Wrm1"].astype(LD)[cand]                                                                  # (n, Hp, D)
    if not c["signed"]:
        V = np.einsum("ns,sj,nsd->njd", qs, SM, np.where(a > 0, r, 0))
        return V * wm
    with np.errstate(invalid="ignore"):
        fac = np.where(a[:, :, None, :] > 0, np.minimum(1, r[:, :, None, :] * wm[:, None, :, :]), 1)      # t = 0: factor 1
    return np.einsum("ns,sj,nsjd->njd", qs, SM, fac)


def energies(c, F):
    """e = (f - prior) / pre1 per column."""
    ns = state_bits(c["masks"], c["Hp"]).sum(axis=1) if c["S"] else np.zeros(0)
    prior = np.concatenate(([0.0], np.ones(c["H"]), ns)).astype(LD) * LD(c["pil_bar"])
    return (np.asarray(F, dtype=LD) - prior[None, :]) / LD(c["pre1"]), np.concatenate(([0.0], np.ones(c["H"]), ns)).astype(LD)


def sigma_cancellation(c, F, q, singles):
    """Per datapoint, the absolute error that the kernels' recovery of an energy from a log-joint puts into sum_k q_k e_k.
    The kernels form e_k = (f_k - pil_bar |s_k|) / pre1 from the float64 f_k = pil_bar |s_k| + pre1 e_k: f_k is rounded once
    or twice (<= 2 u |f_k|), the product pil_bar |s_k| once (u |pil_bar| |s_k|), and the difference of the two is divided by
    pre1 -- an absolute error of at most u (2 |f_k| + |pil_bar| |s_k|) / |pre1| in e_k whatever e_k is.  Weighted with q_k
    and summed: u sum_k q_k (2 |f_k| + |pil_bar| |s_k|) / |pre1|.  `singles`: the singleton columns are recovered this way
    too (the two-pass M-step; the fused pass has their energies directly); the |s| = 0 column never cancels (prior 0)."""
    _, ns = energies(c, F)
    term = np.asarray(q, dtype=LD) * (2 * np.abs(np.asarray(F, dtype=LD)) + abs(LD(c["pil_bar"])) * ns[None, :])
    first = 1 if singles else 1 + c["H"]
    return LD(2.0 ** -53) * term[:, first:].sum(axis=1) / abs(LD(c["pre1"]))


def stats_base(H, D):
    return 3 * H * D + H + NSCALARS


def scatter(c, aid, Y, cand, mult):
    """[Wp_m | Wq_m] (2, H, D) of the datapoints given (each counted mult[n] times)."""
    H, D = c["H"], c["D"]
    out = np.zeros((2, H, D), dtype=LD)
    w = np.asarray(mult, dtype=LD)[:, None, None]
    np.add.at(out[0], cand, aid * Y.astype(LD)[:, None, :] * w)
    np.add.at(out[1], cand, aid * w)
    return out


def packed_stats(c, F, lse1, lseb, keep, mult=None, qcut=None, rows=None):
    """What a call adds to the documented statistics, and the q1 rows.  F, lse1, lseb are those of `rows`; keep is a
    boolean per row; mult counts each row (periodic cases)."""
    H, D = c["H"], c["D"]
    n = F.shape[0]
    mult = np.ones(n) if mult is None else mult
    sl = slice(None) if rows is None else rows
    q = posteriors(c, F, lseb, qcut)
    q[~keep] = 0
    e, ns = energies(c, F)
    w = np.where(keep, mult, 0).astype(LD)
    add = np.zeros(stats_base(H, D), dtype=LD)
    aid = aid_blocks(c, q[:, 1 + H:], rows)
    add[H * D:3 * H * D] = scatter(c, aid, c["Y"][sl], c["cand"][sl], w).reshape(-1)
    add[3 * H * D:3 * H * D + H] = (q[:, 1:1 + H] * w[:, None]).sum(axis=0)
    o = 3 * H * D + H
    add[o] = ((q * ns[None, :]).sum(axis=1) * w).sum()
    add[o + 1] = ((q * e).sum(axis=1) * w).sum()
    add[o + 2] = (np.asarray(lse1, dtype=LD) * w).sum()
    add[o + 3] = w.sum()
    return add, q[:, 1:1 + H], aid


def defer_records(c, F, lse1, lseb, rows=None):
    """(records (n, Hp, D), scalars (n, 4)) of pm_mca_estep_mstats_defer_f64: every datapoint, nothing dropped but exact
    underflow."""
    H = c["H"]
    q = posteriors(c, F, lseb)
    e, ns = energies(c, F)
    sc = np.zeros((F.shape[0], 4), dtype=LD)
    sc[:, 0] = (q * ns[None, :]).sum(axis=1)
    sc[:, 1] = (q * e).sum(axis=1)
    sc[:, 2] = lse1
    return aid_blocks(c, q[:, 1 + H:], rows), sc


def defer_apply(H, D, lseb, cut, Y, cand, rec, sc, q1):
    """(addition to the documented statistics, q1 afterwards) of pm_mca_defer_apply_f64."""
    with np.errstate(invalid="ignore"):
        keep = np.asarray(lseb >= cut)
    add = np.zeros(stats_base(H, D), dtype=LD)
    out = np.zeros((2, H, D), dtype=LD)
    r = np.asarray(rec, dtype=LD)[keep]
    np.add.at(out[0], cand[keep], r * np.asarray(Y, dtype=LD)[keep][:, None, :])
    np.add.at(out[1], cand[keep], r)
    add[H * D:3 * H * D] = out.reshape(-1)
    add[3 * H * D:3 * H * D + H] = np.asarray(q1, dtype=LD)[keep].sum(axis=0)
    o = 3 * H * D + H
    add[o:o + 3] = np.asarray(sc, dtype=LD)[keep][:, :3].sum(axis=0)
    add[o + 3] = keep.sum()
    return add, np.where(keep[:, None], q1, 0.0), keep


def w_update(stats, W, H, D, w_tol):
    """(wt_new, wt_clamped) in float64 arithmetic on operands for which G1 W^2 + Wp_m is exact."""
    HD = H * D
    s = np.asarray(stats, dtype=np.float64)
    w2 = (W * W).reshape(-1)
    wp = s[:HD] * w2 + s[HD:2 * HD]
    wq = np.repeat(s[3 * HD:3 * HD + H], D) * w2 + s[2 * HD:3 * HD]
    small = wq < TINY
    wp = np.where(small, 0.0, wp)
    wq = np.where(small, TINY, wq)
    r = wp / wq
    return r.reshape(H, D), np.maximum(r, w_tol).reshape(H, D)


# --------------------------------------------------------------------------------------------------------------- cases
def state_table(Hp, S, kind):
    """S 16-bit masks over Hp candidate positions.  comb: itertools.combinations order, sizes 2, 3, ... (cycled where S
    exceeds their number); shuffled: the same in a fixed random order; odd: single-candidate rows and a repeated state among
    them."""
    allm = [sum(1 << j for j in cmb) for g in range(2, Hp + 1) for cmb in itertools.combinations(range(Hp), g)]
    if not allm:
        allm = [1]                                 # Hp = 1: only the single-candidate row exists
    m = [allm[i % len(allm)] for i in range(S)]
    if kind == "shuffled":
        m = [m[i] for i in np.random.RandomState(7).permutation(S)]
    elif kind == "odd" and S >= 3:
        m[0] = 1
        m[S // 2] = 1 << (Hp - 1)
        m[-1] = m[1]                               # a repeat (in a paired walk: the second member where S is even)
    return np.array(m, dtype=np.uint16)


# name: (H, D, Hp, S, N, signed, T, table kind, cells).  cells: {plan kind: (DPL, HP, ROOT, paired)}, the instantiation the
# case is meant for (None: PM_ERANGE); MSTEP_ROWS adds (slab, slabs, DPL of the last slab).  T -> rho: 1.0 -> 21 (MCA) / 6
# (MMCA at T <= 1.2), 1.2 -> 6 (MCA), 1.3 -> 13/3.
CASES = {
    # E-step DPL 1 .. 16 x power paths x S edges x tables; two-pass M-step HP 4 .. 16; fused tiles
    "u_d1":      (3, 1, 1, 0, 20, 0, 1.0, "comb", {ESTEP: (1, 1, 21, 0), MSTEP_ROWS: (1, 4, 21, 0, 512, 1, 1), FUSED: (1, 4, 0, 0)}),
    "u_d64":     (7, 64, 2, 1, 20, 0, 1.0, "comb", {ESTEP: (1, 2, 21, 0), MSTEP_ROWS: (1, 4, 21, 0, 512, 1, 1), FUSED: (1, 4, 0, 0)}),
    "u_d65":     (7, 65, 5, 2, 20, 0, 1.2, "comb", {ESTEP: (2, 5, 6, 0), MSTEP_ROWS: (2, 8, 0, 0, 512, 1, 2), FUSED: (2, 8, 0, 0)}),
    "u_d129":    (70, 129, 5, 26, 20, 0, 1.3, "shuffled", {ESTEP: (4, 5, 0, 0), MSTEP_ROWS: (4, 8, 0, 0, 512, 1, 4), FUSED: (4, 8, 0, 0)}),
    "u_d257":    (9, 257, 4, 11, 20, 0, 1.0, "odd", {ESTEP: (8, 4, 21, 0), MSTEP_ROWS: (8, 4, 21, 0, 512, 1, 8), FUSED: (8, 4, 0, 0)}),
    "u_d513":    (6, 513, 4, 3, 10, 0, 1.0, "comb", {ESTEP: (16, 4, 21, 0), MSTEP_ROWS: (8, 4, 21, 0, 512, 2, 1), FUSED: None}),
    "u_d1024":   (17, 1024, 16, 63, 6, 0, 1.3, "comb", {ESTEP: (16, 16, 0, 0), MSTEP_ROWS: (2, 16, 0, 0, 128, 8, 2), FUSED: None}),
    "u_s64":     (130, 33, 8, 64, 20, 0, 1.0, "comb", {ESTEP: (1, 8, 21, 0), MSTEP_ROWS: (1, 8, 21, 0, 512, 1, 1), FUSED: (1, 8, 0, 0)}),
    "u_s65":     (10, 40, 8, 65, 20, 0, 1.2, "shuffled", {ESTEP: (1, 8, 6, 0), MSTEP_ROWS: (1, 8, 0, 0, 512, 1, 1), FUSED: (1, 8, 0, 0)}),
    "u_s129":    (10, 70, 8, 129, 20, 0, 1.0, "odd", {ESTEP: (2, 8, 21, 0), MSTEP_ROWS: (2, 8, 21, 0, 512, 1, 2), FUSED: (2, 8, 0, 0)}),
    "u_hp9":     (11, 257, 9, 84, 12, 0, 1.0, "comb", {ESTEP: (8, 9, 21, 0), MSTEP_ROWS: (4, 12, 21, 0, 256, 2, 1), FUSED: None}),
    "u_hp9_513": (11, 513, 9, 21, 8, 0, 1.3, "comb", {ESTEP: (16, 9, 0, 0), MSTEP_ROWS: (4, 12, 0, 0, 256, 3, 1), FUSED: None}),
    "u_hp12":    (13, 200, 12, 83, 12, 0, 1.0, "comb", {ESTEP: (4, 12, 21, 0), MSTEP_ROWS: (4, 12, 21, 0, 256, 1, 4), FUSED: (4, 12, 0, 0)}),
    "u_hp12_d1": (14, 60, 12, 84, 12, 0, 1.3, "shuffled", {ESTEP: (1, 12, 0, 0), MSTEP_ROWS: (1, 12, 0, 0, 256, 1, 1), FUSED: (1, 12, 0, 0)}),
    "u_hp13":    (14, 129, 13, 40, 12, 0, 1.0, "comb", {ESTEP: (4, 13, 21, 0), MSTEP_ROWS: (2, 16, 21, 0, 128, 2, 1), FUSED: None}),
    "u_hp13_257": (14, 257, 13, 7, 8, 0, 1.3, "odd", {ESTEP: (8, 13, 0, 0), MSTEP_ROWS: (2, 16, 0, 0, 128, 3, 1), FUSED: None}),
    "u_hp16":    (17, 100, 16, 30, 12, 0, 1.0, "shuffled", {ESTEP: (2, 16, 21, 0), MSTEP_ROWS: (2, 16, 21, 0, 128, 1, 2), FUSED: None}),
    "u_hp4_513": (5, 513, 4, 6, 6, 0, 1.3, "comb", {ESTEP: (16, 4, 0, 0), MSTEP_ROWS: (8, 4, 0, 0, 512, 2, 1), FUSED: None}),
    "u_d512":    (6, 512, 4, 5, 8, 0, 1.3, "comb", {ESTEP: (8, 4, 0, 0), MSTEP_ROWS: (8, 4, 0, 0, 512, 1, 8), FUSED: (8, 4, 0, 0)}),
    "u_d128_12": (13, 128, 9, 36, 10, 0, 1.3, "comb", {ESTEP: (2, 9, 0, 0), MSTEP_ROWS: (2, 12, 0, 0, 256, 1, 2), FUSED: (2, 12, 0, 0)}),
    # signed W (MMCA): rho = 6 at T <= 1.2, 13/3 at T = 1.3; the PAIRED tiles are (12, 2), (8, 4), (12, 4)
    "s_d1":      (4, 1, 2, 1, 20, 1, 1.0, "comb", {ESTEP: (1, 2, 6, 0), MSTEP_ROWS: (1, 4, 6, 0, 512, 1, 1), FUSED: (1, 4, 6, 0)}),
    "s_d64":     (70, 64, 4, 11, 20, 1, 1.3, "comb", {ESTEP: (1, 4, 0, 0), MSTEP_ROWS: (1, 4, 0, 0, 512, 1, 1), FUSED: (1, 4, 0, 0)}),
    "s_d65":     (9, 65, 8, 3, 20, 1, 1.0, "shuffled", {ESTEP: (2, 8, 6, 0), MSTEP_ROWS: (2, 8, 6, 0, 512, 1, 2), FUSED: (2, 8, 6, 0)}),
    "s_p8_4":    (9, 129, 5, 26, 16, 1, 1.0, "comb", {ESTEP: (4, 5, 6, 0), MSTEP_ROWS: (4, 8, 6, 0, 512, 1, 4), FUSED: (4, 8, 6, 1)}),
    "s_p8_4_s1": (9, 256, 8, 1, 16, 1, 1.3, "comb", {ESTEP: (4, 8, 0, 0), MSTEP_ROWS: (4, 8, 0, 0, 512, 1, 4), FUSED: (4, 8, 0, 1)}),
    "s_p12_2":   (13, 128, 12, 83, 12, 1, 1.0, "odd", {ESTEP: (2, 12, 6, 0), MSTEP_ROWS: (2, 12, 6, 0, 256, 1, 2), FUSED: (2, 12, 6, 1)}),
    "s_p12_2b":  (13, 65, 9, 84, 12, 1, 1.3, "comb", {ESTEP: (2, 9, 0, 0), MSTEP_ROWS: (2, 12, 0, 0, 256, 1, 2), FUSED: (2, 12, 0, 1)}),
    "s_p12_4":   (130, 129, 9, 3, 12, 1, 1.0, "comb", {ESTEP: (4, 9, 6, 0), MSTEP_ROWS: (4, 12, 6, 0, 256, 1, 4), FUSED: (4, 12, 6, 1)}),
    "s_p12_4b":  (13, 256, 12, 2, 10, 1, 1.3, "comb", {ESTEP: (4, 12, 0, 0), MSTEP_ROWS: (4, 12, 0, 0, 256, 1, 4), FUSED: (4, 12, 0, 1)}),
    "s_d257":    (6, 257, 4, 6, 10, 1, 1.0, "comb", {ESTEP: (8, 4, 6, 0), MSTEP_ROWS: (8, 4, 6, 0, 512, 1, 8), FUSED: (8, 4, 6, 0)}),
    "s_hp12_d1": (13, 33, 12, 40, 12, 1, 1.0, "shuffled", {ESTEP: (1, 12, 6, 0), MSTEP_ROWS: (1, 12, 6, 0, 256, 1, 1), FUSED: (1, 12, 6, 0)}),
    "s_hp16":    (17, 129, 16, 20, 10, 1, 1.0, "comb", {ESTEP: (4, 16, 6, 0), MSTEP_ROWS: (2, 16, 6, 0, 128, 2, 1), FUSED: None}),
    "s_hp13":    (14, 100, 13, 9, 10, 1, 1.3, "odd", {ESTEP: (2, 13, 0, 0), MSTEP_ROWS: (2, 16, 0, 0, 128, 1, 2), FUSED: None}),
    # the remaining (DPL, HP) tiles of each sign and power (tests/test_mca_kernels_cpu.py::test_table_covers_every_cell)
    "u_t2_4":    (6, 128, 4, 11, 12, 0, 1.0, "comb", {ESTEP: (2, 4, 21, 0), MSTEP_ROWS: (2, 4, 21, 0, 512, 1, 2), FUSED: (2, 4, 0, 0)}),
    "u_t4_4":    (5, 129, 4, 6, 12, 0, 1.3, "comb", {ESTEP: (4, 4, 0, 0), MSTEP_ROWS: (4, 4, 0, 0, 512, 1, 4), FUSED: (4, 4, 0, 0)}),
    "u_t4_4b":   (5, 256, 1, 0, 12, 0, 1.0, "comb", {ESTEP: (4, 1, 21, 0), MSTEP_ROWS: (4, 4, 21, 0, 512, 1, 4), FUSED: (4, 4, 0, 0)}),
    "u_t8_8":    (9, 257, 5, 10, 10, 0, 1.0, "comb", {ESTEP: (8, 5, 21, 0), MSTEP_ROWS: (8, 8, 21, 0, 512, 1, 8), FUSED: None}),
    "s_t1_8":    (9, 33, 5, 10, 12, 1, 1.0, "comb", {ESTEP: (1, 5, 6, 0), MSTEP_ROWS: (1, 8, 6, 0, 512, 1, 1), FUSED: (1, 8, 6, 0)}),
    "s_t4_4":    (5, 256, 4, 11, 12, 1, 1.0, "comb", {ESTEP: (4, 4, 6, 0), MSTEP_ROWS: (4, 4, 6, 0, 512, 1, 4), FUSED: (4, 4, 6, 0)}),
    "s_t8_8":    (9, 512, 8, 5, 8, 1, 1.3, "comb", {ESTEP: (8, 8, 0, 0), MSTEP_ROWS: (8, 8, 0, 0, 512, 1, 8), FUSED: None}),
    "s_r1_8":    (9, 64, 8, 28, 12, 1, 1.3, "comb", {ESTEP: (1, 8, 0, 0), MSTEP_ROWS: (1, 8, 0, 0, 512, 1, 1), FUSED: (1, 8, 0, 0)}),
    "s_r1_12":   (13, 20, 9, 36, 12, 1, 1.3, "shuffled", {ESTEP: (1, 9, 0, 0), MSTEP_ROWS: (1, 12, 0, 0, 256, 1, 1), FUSED: (1, 12, 0, 0)}),
    "s_r2_4":    (5, 65, 3, 4, 12, 1, 1.3, "comb", {ESTEP: (2, 3, 0, 0), MSTEP_ROWS: (2, 4, 0, 0, 512, 1, 2), FUSED: (2, 4, 0, 0)}),
    "s_r2_8":    (9, 128, 5, 26, 12, 1, 1.3, "comb", {ESTEP: (2, 5, 0, 0), MSTEP_ROWS: (2, 8, 0, 0, 512, 1, 2), FUSED: (2, 8, 0, 0)}),
    "s_r4_4":    (5, 200, 2, 1, 12, 1, 1.3, "comb", {ESTEP: (4, 2, 0, 0), MSTEP_ROWS: (4, 4, 0, 0, 512, 1, 4), FUSED: (4, 4, 0, 0)}),
    "s_r8_4":    (5, 500, 4, 6, 8, 1, 1.3, "comb", {ESTEP: (8, 4, 0, 0), MSTEP_ROWS: (8, 4, 0, 0, 512, 1, 8), FUSED: (8, 4, 0, 0)}),
    # signed W with exact cancellations: integer-valued W whose rho-th powers cancel in some states (t = 0)
    "s_zero":    (6, 70, 4, 11, 16, 1, 1.0, "comb", {ESTEP: (2, 4, 6, 0), MSTEP_ROWS: (2, 4, 6, 0, 512, 1, 2), FUSED: (2, 4, 6, 0)}),
    "s_zero_p":  (9, 130, 8, 28, 12, 1, 1.0, "comb", {ESTEP: (4, 8, 6, 0), MSTEP_ROWS: (4, 8, 6, 0, 512, 1, 4), FUSED: (4, 8, 6, 1)}),
    # the second trip of the grid-capped datapoint loops: N = 4 * 2048 + 5, rows periodic with period 13
    "u_trip2":   (3, 3, 2, 1, 8197, 0, 1.0, "comb", {ESTEP: (1, 2, 21, 0), MSTEP_ROWS: (1, 4, 21, 0, 512, 1, 1), FUSED: (1, 4, 0, 0)}),
    "s_trip2":   (3, 3, 2, 1, 8197, 1, 1.0, "comb", {ESTEP: (1, 2, 6, 0), MSTEP_ROWS: (1, 4, 6, 0, 512, 1, 1), FUSED: (1, 4, 6, 0)}),
}
PERIOD = 13
MCA_T_BOUND, MMCA_T_BOUND = 1.05, 1.2


def make_case(name, hot):
    """Operands of a case as the C ABI takes them.  HOT: pre1 = -2^-24 and a flat prior (pil_bar = 0) put all weights of a
    row within a factor e.  COLD: pil_bar = -1.5 and pre1 such that the median multi-cause state of a row
    lies at the cut-offs (beta (f - max f) = -745): states on both sides of each."""
    H, D, Hp, S, N, signed, T, kind, cells = CASES[name]
    rng = np.random.RandomState(sum(map(ord, name)))
    rows = min(N, PERIOD)
    rho = rho_of(T, MMCA_T_BOUND if signed else MCA_T_BOUND)
    if name.startswith("s_zero"):
        # +-1 and +-2 in matching columns: |W|^rho is exact (powers of two), sums of opposite signs cancel exactly
        W = rng.choice([-2.0, -1.0, 1.0, 2.0], size=(H, D))
        W[1] = -W[0]
        W[2, ::2] = -W[0, ::2]
    elif signed:
        W = rng.uniform(0.3, 2.0, size=(H, D)) * rng.choice([-1.0, 1.0], size=(H, D))
    else:
        W = rng.uniform(0.3, 2.0, size=(H, D))
    candr = np.stack([rng.permutation(H)[:Hp] for _ in range(rows)]).astype(np.int32)
    if name.startswith("s_zero"):
        candr[:, 0], candr[:, 1] = 0, 1            # every datapoint holds the cancelling pair in its first state
        for r in range(rows):
            rest = [h for h in rng.permutation(H) if h > 1][:Hp - 2]
            candr[r, 2:] = rest
    masks = state_table(Hp, S, kind)
    wrho, wrm1, wn = tables(W, rho, signed)
    # a datapoint is the max-superposition Wbar of one of ITS states (row r: state 3 r + 1; without states: its first
    # candidate) plus noise, so that in the COLD runs a multi-cause state carries the weight and the others fall away from it
    Yr = rng.uniform(-0.1, 0.1, size=(rows, D))
    for r in range(rows):
        if S and not (S < 20 and r % 2):          # (small tables: every other datapoint is a single cause, its states unlikely)
            t = wrho[candr[r][state_bits(masks[(3 * r + 1) % S:][:1], Hp)[0] == 1]].sum(axis=0)
            Yr[r] += np.sign(t) * np.abs(t) ** (1.0 / rho)
        else:
            Yr[r] += W[candr[r, 0]]
    rep = -(-N // rows)
    Y = np.tile(Yr, (rep, 1))[:N]
    cand = np.tile(candr, (rep, 1))[:N]
    c = dict(name=name, hot=hot, H=H, D=D, Hp=Hp, S=S, N=N, rows=rows, signed=signed, T=T, rho=rho, inv_rho=1.0 / rho,
             beta=1.0 / T, kind=kind, cells=cells, W=W, Y=Y, cand=cand, masks=masks, Wrho=wrho, Wrm1=wrm1, wnorm2=wn,
             ynorm2=(Y.astype(LD) ** 2).sum(axis=1).astype(np.float64),
             scores=(Y.astype(LD) @ W.astype(LD).T).astype(np.float64), pil_bar=0.0, pre1=-2.0 ** -24)
    if not hot:
        c["pil_bar"], c["pre1"] = 0.0, -1.0         # (the energies alone: only they scale with pre1)
        F = logpj(c, slice(0, rows))
        c["pil_bar"] = -1.5
        # at pre1 = -1: the rows' largest term above their median state; a table of fewer than 20 states may hold the best
        # one only (a gap near 0): there the rows' WORST state is put at 1.5 times the cut-offs, without states half the row's
        # whole spread at them
        if S >= 20:
            low = np.median(F[:, 1 + H:], axis=1)
        elif S:
            low = F.max(axis=1) - (F.max(axis=1) - F[:, 1 + H:].min(axis=1)) / 1.5
        else:
            low = (F.max(axis=1) + F.min(axis=1)) / 2
        gap = float((np.median if S >= 20 else np.max)(F.max(axis=1) - low))     # (small tables: the datapoint that spreads most)
        c["pre1"] = -(745.0 * T) / max(gap, 1e-3)             # ... put at the cut-offs: beta (f - max) = -745 there
        k = exponent_conditioning(dict(c, rows=rows), logpj(c, slice(0, rows)))
        if k > 1.8e-11:                                    # (linear in pre1: keep float64's own error of an exponent below 2e-11)
            c["pre1"] *= 1.8e-11 / k
    return c


def exponent_conditioning(c, F):
    """Worst-case absolute float64 error of an exponent beta f - lseb of a case: the Gram identity |W_h|^2 - 2 <W_h, y> + |y|^2
    rounds each of its three terms and two sums (<= 3 u of their magnitudes, times beta |pre1|), a log-joint and the
    product with beta round once each (2 u |beta f|).  The 1e-11 bounds on posterior weights presuppose that this stays
    of that order: the table's shapes are chosen so (tests/test_mca_kernels_cpu.py asserts <= 2e-11 for every case)."""
    u = 2.0 ** -53
    r = slice(0, c["rows"])
    gram = float((c["wnorm2"][None, :] + 2 * np.abs(c["scores"][r]) + c["ynorm2"][r][:, None]).max())
    return c["beta"] * abs(c["pre1"]) * gram * 3 * u + 2 * u * float(np.abs(c["beta"] * np.asarray(F, dtype=np.float64)).max())


def case_reference(c):
    """Log-joints and log-evidences of the distinct rows, longdouble and rounded; computed once per case."""
    r = slice(0, c["rows"])
    F = logpj(c, r)
    l1, lb = lse(F, c["beta"])
    return dict(F=F, lse1=l1, lseb=lb, F64=F.astype(np.float64), lse1_64=l1.astype(np.float64), lseb_64=lb.astype(np.float64))


def tile(c, x):
    """Rows of the distinct datapoints -> all N."""
    x = np.asarray(x)
    rep = -(-c["N"] // c["rows"])
    return np.tile(x, (rep,) + (1,) * (x.ndim - 1))[:c["N"]]


def mult(c):
    return np.bincount(np.arange(c["N"]) % c["rows"], minlength=c["rows"])


# ------------------------------------------------------------------------------ the rescaling branch of the fused pass
# name: (base case, sizes of the states in table order, the states at which the lazy reference level moves)
RESCALE = {
    "resc_u_first": ("u_s65", (2, 3, 2, 2, 2), (0, 1)),
    "resc_u_mid": ("u_s65", (2, 2, 2, 3, 2, 2, 2), (0, 3)),
    "resc_u_last": ("u_s65", (2, 2, 2, 2, 3), (0, 4)),
    "resc_p_first": ("s_p8_4", (2, 3, 2), (0, 1)),                     # paired tile: the second state of the first trip
    "resc_p_both": ("s_p8_4", (2, 2, 3, 4, 2, 2), (0, 2, 3)),          # both states of a trip
    "resc_p_second": ("s_p8_4", (2, 2, 2, 3, 2, 2), (0, 3)),           # the second only
    "resc_p_last": ("s_p8_4", (2, 2, 2, 2, 3), (0, 4)),                # the odd end: the first state of the last trip
}


def make_rescale_case(name):
    """A HOT case whose prior pil_bar = 64 T makes beta f_s = 64 |s| + O(1e-4): the table's order of state sizes alone
    decides where beta f_s exceeds the lazy maximum by more than 50.  With pre1 = -2^-24 these are also the cases where the
    kernels' recovery of a state's energy from its log-joint cancels most (sigma_cancellation)."""
    base, sizes, _ = RESCALE[name]
    c = make_case(base, True)
    used = {}
    masks = []
    for g in sizes:
        k = used.get(g, 0)
        used[g] = k + 1
        masks.append(sum(1 << j for j in list(itertools.combinations(range(c["Hp"]), g))[k]))
    c.update(name=name, masks=np.array(masks, dtype=np.uint16), S=len(masks), pil_bar=64.0 * c["T"], kind="rescale")
    return c


def rescale_points(c, ref):
    """The states at which `bf > M + 50` holds for the lazily followed maximum M of the fused pass; the same for every row."""
    out = set()
    for row in np.asarray(ref["F"])[:, 1 + c["H"]:]:
        M, pts = -np.inf, []
        for s, f in enumerate(row):
            bf = float(c["beta"] * f)
            if bf > M + 50.0:
                M = bf
                pts.append(s)
        out.add(tuple(pts))
    assert len(out) == 1, out
    return out.pop()
