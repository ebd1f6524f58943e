"""Plain NumPy statements of what the entry points of dsc_kernels.hip compute (Discrete / Ternary Sparse Coding), written
from the semantics include/prosper_hip.h documents for dsc_et.py / tsc_et.py -- a loop over the datapoints, sums over states and
positions, np.longdouble wherever something rounds.  Nothing here follows the kernels' tables, tiles or lane layouts.

Inputs are the operands of the C ABI: scores A (N, H) = Y W^T, the Gram matrix G (H, H) = W W^T, ynorm2 (N,), candidates
cand (N, H') (repeats allowed), the state table state_idx (S, H') of indices into `values`, the log-prior table `prior`
(Kt,), and the scalars of pm_dsc_params.  Columns of the log-joints: [null | singletons by non-zero value then latent |
states], or the states only under PM_DSC_TABLE_ONLY.

Pinned on oracle/dsc_oracle.py and oracle/tsc_oracle.py by tests/test_dsc_kernels_cpu.py."""
import numpy as np

LD = np.longdouble
MAX_K = 8                 # PM_DSC_MAX_K
NZ_MAX = 16               # PM_BSC_NZ_MAX
NZ_PAD = 0xFFFF
TABLE_ONLY, LAST_POSITION = 1, 2


def nonzero_values(values, K0):
    """The non-zero latent values in the order of their singleton blocks."""
    return [(k, values[k]) for k in range(len(values)) if k != K0]


# ------------------------------------------------------------------------------------------------------------ selection
def dsc_select_scores(A, G, values, K0, logpi, pre1):
    """R[n, h] = -max_{k != K0} (pre1 (v_k^2 G_hh - 2 v_k A[n, h]) + log pi_k)."""
    A = np.asarray(A, dtype=LD)
    w2 = np.diag(G).astype(LD)
    best = np.full(A.shape, -np.inf, dtype=LD)
    for k, v in nonzero_values(values, K0):
        best = np.maximum(best, LD(pre1) * (LD(v) * LD(v) * w2[None, :] - LD(2) * LD(v) * A) + LD(logpi[k]))
    return -best


def tsc_select_scores(A, G):
    """R (N, 2H): minus the squared distance (up to |y|^2) of every one-cause state, the -1 block, then the +1 block."""
    A = np.asarray(A, dtype=LD)
    w2 = np.diag(G).astype(LD)
    return np.concatenate([-(w2[None, :] + 2 * A), -(w2[None, :] - 2 * A)], axis=1)


def rank_smallest_first(R, Hp):
    """The H' smallest of every row, best first; equal values rank by index, the smaller first (a stable argsort)."""
    return np.argsort(R, axis=1, kind="stable")[:, :Hp].astype(np.int64)


def rank_largest_best_last(R, Hp):
    """The H' largest of every row in ascending order (best last); of equal values the larger index ranks higher (the tail
    of a stable ascending argsort)."""
    return np.argsort(R, axis=1, kind="stable")[:, -Hp:].astype(np.int64)


def dsc_candidates(A, G, values, K0, logpi, pre1, Hp):
    return rank_smallest_first(dsc_select_scores(A, G, values, K0, logpi, pre1), Hp)


def tsc_candidates(A, G, Hp):
    """One-cause states ranked, stored as latents (state % H): a latent may occur twice."""
    return rank_largest_best_last(tsc_select_scores(A, G), Hp) % np.asarray(A).shape[1]


# --------------------------------------------------------------------------------------------------------------- E-step
def state_matrix(values, state_idx):
    """(S, H') latent values of the multi-cause states."""
    idx = np.asarray(state_idx, dtype=np.int64).reshape(-1, np.asarray(state_idx).shape[-1])
    return np.asarray(values, dtype=LD)[idx]


def energies(A, G, yn, cand, values, K0, state_idx, flags):
    """|y - W^T s|^2 of every column's state through A and G (longdouble): (N, Kt)."""
    A, G, yn = np.asarray(A, dtype=LD), np.asarray(G, dtype=LD), np.asarray(yn, dtype=LD)
    N, H = A.shape
    SM = state_matrix(values, state_idx)
    S, Hp = SM.shape
    cols = []
    if not flags & TABLE_ONLY:
        cols.append(yn[:, None])
        w2 = np.diag(G)
        for _, v in nonzero_values(values, K0):
            cols.append(LD(v) * LD(v) * w2[None, :] - 2 * LD(v) * A + yn[:, None])
    E = np.zeros((N, S), dtype=LD)
    for n in range(N):
        c = np.asarray(cand[n], dtype=np.int64)
        a, g = A[n, c], G[np.ix_(c, c)]
        E[n] = yn[n] - 2 * (SM @ a) + ((SM @ g) * SM).sum(axis=1)            # |y|^2 - 2 v.a + v^T g v of every state
    cols.append(E)
    return np.concatenate(cols, axis=1)


def log_joints(E, prior, ecoef, pscale):
    """ecoef e + pscale prior, longdouble."""
    return LD(ecoef) * np.asarray(E, dtype=LD) + LD(pscale) * np.asarray(prior, dtype=LD)[None, :]


def lse(F):
    """Row-wise log sum exp in longdouble."""
    F = np.asarray(F, dtype=LD)
    m = F.max(axis=1)
    return m + np.log(np.exp(F - m[:, None]).sum(axis=1))


def weights(F, l):
    """Posterior weights exp(F - lse), longdouble."""
    return np.exp(np.asarray(F, dtype=LD) - np.asarray(l, dtype=LD)[:, None])


def dropped_below(F64, against, cut):
    """Columns with F64 - against[n] > cut false, in float64 as the kernels evaluate it (exact operands: the same bits)."""
    with np.errstate(invalid="ignore"):
        return ~(np.asarray(F64, dtype=np.float64) - np.asarray(against, dtype=np.float64)[:, None] > cut)


def last_positions(c):
    """True where position j holds the LAST occurrence of its latent among the candidates c."""
    c = list(c)
    return np.array([c[j] not in c[j + 1:] for j in range(len(c))])


# --------------------------------------------------------------------------------------------------------------- M-step
def stats_len(H, D):
    return H * D + H * H + H + MAX_K + 4


def row_stats(F, l, keep, E, cand, values, K0, state_idx, flags, H, D, lists=True, mult=None, drop=None):
    """The per-datapoint part of the M-step for the rows with keep[n]: posterior weights q = exp(F - l).  ``mult[n]``: how many
    datapoints are copies of row n (default one each): the sums count a row that often.  ``drop`` (N, Kt) bool: columns whose
    weight counts as zero -- the kernels leave out what lies below e^-37 of a row's largest term (the one-pass statistics)
    or below e^-60 of its evidence (the row pass); see ``dropped_below``.

    Returns a dict:  expect (N, H) E[s] rows (zero rows where not kept);  nz_idx / nz_cnt: the ascending non-zero latents of
    every row, the first NZ_MAX kept, the rest of the 16 slots NZ_PAD;  stats: the packed statistics (longdouble; the Wp
    section stays zero): Wq upper triangle (the candidates' second moments: position pair (a, b), a <= b, lands at
    (min, max) of its two latents; under LAST_POSITION only pairs of last occurrences), qdiag (the singletons' second
    moments), the value counts (entry K0 unused; every position counts, masked or not), sum q e, sum lse, kept, rows whose
    list overflowed."""
    F, E = np.asarray(F, dtype=LD), np.asarray(E, dtype=LD)
    N, Kt = F.shape
    SM = state_matrix(values, state_idx)
    sidx = np.asarray(state_idx, dtype=np.int64).reshape(SM.shape)
    S, Hp = SM.shape
    tab = bool(flags & TABLE_ONLY)
    base = 0 if tab else 1 + (len(values) - 1) * H
    assert Kt == base + S
    expect = np.zeros((N, H), dtype=LD)
    st = np.zeros(stats_len(H, D), dtype=LD)
    Wq = st[H * D:H * D + H * H].reshape(H, H)
    qdiag = st[H * D + H * H:H * D + H * H + H]
    cnt = st[H * D + H * H + H:H * D + H * H + H + MAX_K]
    scal = st[H * D + H * H + H + MAX_K:]
    mult = np.ones(N, dtype=np.int64) if mult is None else np.asarray(mult)
    for n in range(N):
        if not keep[n]:
            continue
        w = LD(int(mult[n]))
        q = np.exp(F[n] - LD(l[n]))
        if drop is not None:
            q = np.where(drop[n], LD(0), q)
        scal[0] += w * (q * E[n]).sum()
        scal[1] += w * LD(l[n])
        scal[2] += w
        if not tab:
            for c, (k, v) in enumerate(nonzero_values(values, K0)):
                q1 = q[1 + c * H:1 + (c + 1) * H]
                expect[n] += q1 * LD(v)
                qdiag += w * q1 * LD(v) * LD(v)
                cnt[k] += w * q1.sum()
        qs = q[base:]
        cn = np.asarray(cand[n], dtype=np.int64)
        last = last_positions(cn) if flags & LAST_POSITION else np.ones(Hp, dtype=bool)
        for k in range(len(values)):
            if k != K0:
                cnt[k] += w * (qs * (sidx == k).sum(axis=1)).sum()
        m = qs @ SM                                          # (H',): E[s] of every candidate position (SM is 0 at K0)
        B = (SM * qs[:, None]).T @ SM                        # (H', H'): second moments of the positions
        for a in range(Hp):
            if not last[a]:
                continue
            expect[n, cn[a]] += m[a]
            for b in range(a, Hp):
                if last[b]:
                    Wq[min(cn[a], cn[b]), max(cn[a], cn[b])] += w * B[a, b]
    out = {"expect": expect, "stats": st}
    if lists:
        idx = np.full((N, NZ_MAX), NZ_PAD, dtype=np.int64)
        count = np.zeros(N, dtype=np.int64)
        for n in range(N):
            nz = np.nonzero(expect[n] != 0)[0]
            count[n] = len(nz)
            idx[n, :min(len(nz), NZ_MAX)] = nz[:NZ_MAX]
            if keep[n] and len(nz) > NZ_MAX:
                scal[3] += int(mult[n])
        out["nz_idx"], out["nz_cnt"] = idx, count
    return out


# ---------------------------------------------------------------------------------------------------------------------
# The shapes and data of tests/test_dsc_kernels_gpu.py (tests/test_dsc_kernels_cpu.py pins the plan of every shape, the
# exactness of its arithmetic and the spread of its posterior weights without a device).
# ---------------------------------------------------------------------------------------------------------------------
ESTEP, MSTATS, ROWS = 0, 1, 2           # PM_DSC_PLAN_ESTEP / _ESTEP_MSTATS / _MSTEP_ROWS
L16, WAVE = 1, 2                        # PM_DSC_PLAN_LANES16 / _WAVE
T3 = TABLE_ONLY | LAST_POSITION
SWEEP_PERIOD = 67                       # rows of a sweep case repeat with this period (prime: no multiple of a tile or a sweep)

# name: (H, H', K, K0, S, N, D, flags, state table kind,
#        plan of estep, estep_mstats, mstep_rows as (family, MAXHP, VPL, KM, stage, NT); None: PM_ERANGE)
# Table kinds: "le3" at most three non-zero positions per state, "four" the same with one state of four, "tsc" a null
# state and one-cause states among them (PM_DSC_TABLE_ONLY tables hold those).  Candidates repeat where flags has
# PM_DSC_LAST_POSITION.  N > 1000: a few rows past two grid sweeps of every entry (the CPU module reads the sweep from the
# plan's grid size).
CASES = {
    # sixteen lanes per datapoint, the four <MAXHP, VPL> instantiations
    "l16_8_8": (17, 3, 3, 1, 7, 17, 3, 0, "le3",
                (L16, 8, 8, 0, 1, 19), (L16, 8, 8, 4, 1, 19), (L16, 8, 8, 8, 1, 0)),
    "l16_8_16": (129, 8, 3, 0, 17, 15, 1, 0, "le3",
                 (L16, 8, 16, 0, 1, 129), (L16, 8, 16, 4, 1, 129), (L16, 8, 16, 8, 1, 0)),
    "l16_16_8": (24, 9, 2, 1, 15, 16, 3, 0, "le3",
                 (L16, 16, 8, 0, 1, 46), (L16, 16, 8, 4, 1, 46), (L16, 16, 8, 8, 1, 0)),
    "l16_16_16": (129, 9, 2, 0, 16, 67, 1, 0, "le3",
                  (L16, 16, 16, 0, 1, 46), (L16, 16, 16, 4, 1, 46), (L16, 16, 16, 8, 1, 0)),
    # KM = PM_DSC_MAX_K; NT = 0 because 1 + 6 * 4 + 15 * 16 = 265 > 256 with S > 0
    "km8_nt_over": (17, 6, 5, 2, 15, 17, 3, 0, "le3",
                    (L16, 8, 8, 0, 1, 0), (L16, 8, 8, 8, 1, 0), (L16, 8, 8, 8, 1, 0)),
    "km8_16_16": (256, 9, 5, 4, 17, 15, 1, 0, "le3",
                  (L16, 16, 16, 0, 1, 0), (L16, 16, 16, 8, 1, 0), (WAVE, 16, 0, 8, 1, 0)),
    "k8": (128, 8, 8, 3, 17, 16, 1, 0, "le3",
           (L16, 8, 8, 0, 1, 0), (L16, 8, 8, 8, 1, 0), (L16, 8, 8, 8, 1, 0)),
    "k4_h15": (15, 2, 4, 3, 1, 1, 3, 0, "le3",
               (L16, 8, 8, 0, 1, 16), (L16, 8, 8, 4, 1, 16), (L16, 8, 8, 8, 1, 0)),
    # NT = 0 because S = 0; the smallest problem
    "s0": (17, 3, 3, 2, 0, 17, 3, 0, "le3",
           (L16, 8, 8, 0, 1, 0), (L16, 8, 8, 4, 1, 0), (L16, 8, 8, 8, 1, 0)),
    "h1": (1, 1, 2, 0, 1, 1, 1, 0, "le3",
           (L16, 8, 8, 0, 1, 2), (L16, 8, 8, 4, 1, 2), (L16, 8, 8, 8, 1, 0)),
    # the prior table no longer fits the LDS budget: read from global memory
    "stage_off": (128, 4, 3, 1, 2000, 17, 1, 0, "le3",
                  (L16, 8, 8, 0, 0, 33), (L16, 8, 8, 4, 0, 33), (L16, 8, 8, 8, 0, 0)),
    "stage_off_16": (256, 4, 2, 0, 2500, 5, 1, 0, "le3",
                     (L16, 8, 16, 0, 0, 11), (L16, 8, 16, 4, 0, 11), (WAVE, 8, 0, 8, 0, 0)),
    # the in-kernel fall-back from the energy-term tables, beside the same shape without it
    "le3": (17, 4, 3, 1, 40, 17, 3, 0, "le3",
            (L16, 8, 8, 0, 1, 33), (L16, 8, 8, 4, 1, 33), (L16, 8, 8, 8, 1, 0)),
    "too_many": (17, 4, 3, 1, 40, 17, 3, 0, "four",
                 (L16, 8, 8, 0, 1, 33), (L16, 8, 8, 4, 1, 33), (L16, 8, 8, 8, 1, 0)),
    "too_many_wave": (257, 4, 3, 1, 40, 5, 1, 0, "four",
                      (WAVE, 8, 0, 0, 1, 33), None, (WAVE, 8, 0, 8, 1, 0)),
    # lists: exactly PM_BSC_NZ_MAX non-zeros (H = 16) and one more (H = 17) with positive values
    "nz17": (17, 2, 2, 0, 1, 16, 1, 0, "le3",
             (L16, 8, 8, 0, 1, 4), (L16, 8, 8, 4, 1, 4), (L16, 8, 8, 8, 1, 0)),
    # one wavefront per datapoint: H > 256 ...
    "wave8_h257": (257, 3, 3, 2, 7, 17, 3, 0, "le3",
                   (WAVE, 8, 0, 0, 1, 19), None, (WAVE, 8, 0, 8, 1, 0)),
    "wave16_h257": (257, 9, 2, 1, 16, 15, 1, 0, "le3",
                    (WAVE, 16, 0, 0, 1, 46), None, (WAVE, 16, 0, 8, 1, 0)),
    # ... and H <= 256 where the sixteen-lane layout passes 40 KB (each entry has its own layout)
    "wave8_lds_e": (256, 8, 3, 0, 700, 5, 1, 0, "le3",
                    (WAVE, 8, 0, 0, 0, 129), None, (WAVE, 8, 0, 8, 1, 0)),
    "wave8_lds_m": (250, 8, 3, 2, 17, 16, 1, 0, "le3",
                    (L16, 8, 16, 0, 1, 129), (L16, 8, 16, 4, 1, 129), (WAVE, 8, 0, 8, 1, 0)),
    "wave16_lds_e": (16, 16, 2, 1, 16, 17, 3, 0, "le3",
                     (WAVE, 16, 0, 0, 1, 137), None, (L16, 16, 8, 8, 1, 0)),
    "wave16_lds_m": (48, 16, 2, 0, 16, 15, 1, 0, "le3",
                     (WAVE, 16, 0, 0, 1, 137), None, (WAVE, 16, 0, 8, 1, 0)),
    # Ternary Sparse Coding: table-only columns, repeated candidates, last-position rule; both families
    "tsc_l16": (16, 4, 3, 1, 17, 17, 3, T3, "tsc",
                (L16, 8, 8, 0, 1, 33), (L16, 8, 8, 4, 1, 33), (L16, 8, 8, 8, 1, 0)),
    "tsc_l16_16": (129, 9, 3, 1, 15, 16, 1, T3, "tsc",
                   (L16, 16, 16, 0, 1, 163), (L16, 16, 16, 4, 1, 163), (L16, 16, 16, 8, 1, 0)),
    "tsc_wave": (257, 3, 3, 1, 7, 15, 1, T3, "tsc",
                 (WAVE, 8, 0, 0, 1, 19), None, (WAVE, 8, 0, 8, 1, 0)),
    # a few rows past two full grid sweeps, per kernel family (H <= 17, D <= 3)
    "sweep_l16": (5, 2, 2, 0, 1, 32773, 3, 0, "le3",
                  (L16, 8, 8, 0, 1, 4), (L16, 8, 8, 4, 1, 4), (L16, 8, 8, 8, 1, 0)),
    "sweep_wave": (17, 16, 2, 1, 240, 8197, 1, 0, "le3",
                   (WAVE, 16, 0, 0, 1, 137), None, (WAVE, 16, 0, 8, 1, 0)),
}

VALUE_POOL = [1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 4.0]


def ints(rows, cols, seed, lo=-8, hi=8):
    """Position-dependent integers in [lo, hi] as f64 (tests/test_eval_kernels_gpu.py: not symmetric, so a transposed or
    shifted tile map changes the answer)."""
    rng = np.random.RandomState(seed)
    i, j = np.arange(rows)[:, None], np.arange(cols)[None, :]
    return (lo + (rng.randint(0, hi - lo + 1, size=(rows, cols)) + (i + 3 * j) % 5) % (hi - lo + 1)).astype(np.float64)


def case_values(K, K0):
    """K latent values, the zero at K0, the others the first K - 1 of VALUE_POOL (K = 2: the single value 1)."""
    v = list(VALUE_POOL[:K - 1])
    v.insert(K0, 0.0)
    return np.array(v)


def state_table(kind, S, Hp, K, K0, seed):
    """(S, H') uint8 indices into the values: random, distinct non-zero positions per state."""
    rng = np.random.RandomState(seed)
    nzk = [k for k in range(K) if k != K0]
    tab = np.full((S, Hp), K0, dtype=np.uint8)
    for s in range(S):
        g = min(Hp, 2 + (s % 2))                              # two or three non-zero positions
        if kind == "tsc":
            g = min(Hp, s % 4)                                # the null state, one, two and three causes
        if kind == "four" and s == S // 2:
            g = 4
        pos = rng.permutation(Hp)[:g]
        tab[s, pos] = rng.choice(nzk, size=g)
    return tab


def make_case(name, hot, seed=0):
    """The operands of a case as a dict: A, G (symmetric, non-constant, a Gram matrix is), yn, cand, values, state_idx,
    prior, ecoef, pscale, and the shape.  Everything is a small integer or a dyadic fraction: see ``exact``.  ``hot``:
    ecoef = -2^-20 and a flat prior -- all posterior weights of a row within a factor e; else ecoef = -2, pscale = 0.5
    and a position-dependent prior -- terms below the kernels' e^-37 / e^-60 cut-offs occur."""
    H, Hp, K, K0, S, N, D, flags, kind = CASES[name][:9]
    sd = seed + 1000 * (sum(map(ord, name)) % 97)
    rows = min(N, SWEEP_PERIOD) if N > 1000 else N
    rng = np.random.RandomState(sd)
    A = ints(rows, H, sd + 1)
    M = ints(H, H, sd + 2, -2, 2)
    G = M + M.T
    G[np.arange(H), np.arange(H)] = 1.0 + (np.arange(H) * 5 + sd) % 9                  # |W_h|^2 > 0, position-dependent
    yn = ints(1, rows, sd + 3, 0, 40)[0]
    if flags & LAST_POSITION:
        cand = rng.randint(0, min(H, Hp + 1), size=(rows, Hp)) * max(1, (H - 1) // (Hp + 1))   # few latents: repeats
        cand[0] = cand[0, 0]                                                             # one row: a single latent
    else:
        cand = np.stack([rng.permutation(H)[:Hp] for _ in range(rows)])
    values = case_values(K, K0)
    tab = state_table(kind, S, Hp, K, K0, sd + 4)
    Kt = S if flags & TABLE_ONLY else 1 + (K - 1) * H + S
    if hot:
        ecoef, pscale, prior = -2.0 ** -20, 1.0, np.full(Kt, -1.5)
    else:
        ecoef, pscale, prior = -2.0, 0.5, -((np.arange(Kt) * 7 + 3) % 64) / 16.0
    rep = -(-N // rows)
    t = (lambda x: np.tile(x, (rep,) + (1,) * (x.ndim - 1))[:N])
    return dict(name=name, H=H, Hp=Hp, K=K, K0=K0, S=S, N=N, D=D, flags=flags, Kt=Kt, rows=rows, hot=hot,
                A=t(A), G=G, yn=t(yn), cand=t(cand.astype(np.int32)), values=values, state_idx=tab, prior=prior, ecoef=ecoef,
                pscale=pscale)


def case_reference(c):
    """Energies, log-joints (longdouble and, exactly, float64) and lse of the distinct rows of a case, tiled to N rows."""
    r = c["rows"]
    E = energies(c["A"][:r], c["G"], c["yn"][:r], c["cand"][:r], c["values"], c["K0"], c["state_idx"], c["flags"])
    F = log_joints(E, c["prior"], c["ecoef"], c["pscale"])
    F64 = c["ecoef"] * E.astype(np.float64) + c["pscale"] * c["prior"][None, :]
    exact = bool(np.abs(E).max() < 2.0 ** 30 and (E == np.rint(E)).all() and (F64.astype(LD) == F).all()) if F.size else True
    rep = -(-c["N"] // r)
    t = (lambda x: np.tile(x, (rep,) + (1,) * (x.ndim - 1))[:c["N"]])
    return dict(E=t(E), F=t(F), F64=t(F64), lse=t(lse(F)) if F.shape[1] else None, exact=exact)


def lse_bound(Kt, l):
    """|lse_kernel - lse| allowed (derivation: the docstring of tests/test_dsc_kernels_gpu.py)."""
    u = 2.0 ** -53
    per_lane = -(-Kt // 16) + 6
    rounding = (2.3e-16 + per_lane * u) + 4 * u * max(1.0, np.log(Kt)) + 2 * u * np.abs(l)
    return 4 * rounding + Kt * np.exp(-37.0)
