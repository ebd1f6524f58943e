"""Plain NumPy statements of what the Binary Sparse Coding entry points compute (bsc_kernels.hip, bsc_rows16.hip,
bsc_fused.hip, bsc_fused8.hip, bsc_wp_sparse.hip), written from the lines of the reference project's bsc_et.py that
include/prosper_hip.h cites -- select_Hprimes :98-115, E_step :119-192, M_step :247-272, :334-366, :395-415 -- as loops over
datapoints and sums over states, np.longdouble wherever something rounds.  Nothing here follows the kernels' tables, tiles,
lane layouts or their Gram-matrix algebra: energies are |y - mu - W^T s|^2 taken from the vectors themselves.

Operands are those of the C ABI: Y (N, D) data, Wt (H, D) = W^T, mu (D) or None, candidates cand (N, H') (best last), the
state matrix SM (S, H') of generate_state_matrix (camodels/__init__.py:21-47: all states of 2 .. gamma causes, by size, each
size in the order of itertools.combinations), and the scalars of pm_bsc_estep_params.  Columns of the log-joints:
[null | singletons h = 0 .. H-1 | multi-cause states].

What the kernels document as left out, and the reference leaves out with them (exact operands: both sides take the same
decisions, the comparisons below run in float64 on the same bits):
  NEGLIGIBLE = -37   bsc_rows16_body.h, bsc_fused8.hip ("only terms within exp(-37) of the largest are evaluated"): in the
                     one-pass kernels (pm_bsc_select_estep_f64, pm_bsc_estep_fused_f64, pm_bsc_estep_fused8*_f64) a term with
                     f <= max_k f_k - 37 adds nothing to the log-sum-exp, to E[s] or to a statistic
  QCUT = -50         bsc_rows16.hip, bsc_mstep_rows16_kernel ("exp(-50) ~ 2e-22: below every statistic's rounding"): a term
                     with f - lse <= -50 adds nothing
  the generic kernels of bsc_kernels.hip leave nothing out.

Statistics come in the pieces the three documented diagonal conventions are assembled from (``row_stats``): q1 (the singletons'
column sums), m1 (the multi-cause states' share of E[s]), the strict upper pair block.
  pm_bsc_mstep_rows_f64 / _rows16_f64:     qdiag = q1, diag(Wq block) = m1, mus = q1 + m1
  pm_bsc_estep_fused_f64:                  qdiag untouched, diag(Wq block) = m1, mus = q1 + m1
  pm_bsc_estep_fused8*_f64, defer_apply:   qdiag = mus = q1 + m1, diag(Wq block) untouched

The lse bound (``lse_bound``), derived.  u = 2^-53.  f_k - m is exact (multiples of 2^-20 below 2^17).  pm_exp_tab documents
2.3e-16 relative error per term (exp_lds of bsc_fused8.hip the same; the generic kernels call exp).  A lane adds at most
T = ceil(K / L) terms one after the other (L lanes per datapoint: 16 in bsc_rows16_body.h, 32 in bsc_fused8.hip, 64 in
bsc_kernels.hip, whose online form also rescales the running sum by one more exponential per step), then the lanes are summed
in log2 L steps: every step rounds once and carries at most two exponentials, so the sum is off by at most
(T + log2 L) (2 * 2.3e-16 + 2 u) relative.  Terms at or below e^-37 of the largest are dropped: at most K e^-37 relative to a
sum >= 1.  log (log_ge1: "relative error ~2e-16", on [1, K]) turns a relative error of its argument into an absolute one and
adds 2e-16 max(1, log K) of its own; the final addition and the reference's cast to float64 round to u |lse| each.  With a
factor 4 on the rounding part:
    |lse - ref| <= 4 ((T + log2 L) (4.6e-16 + 2 u) + 2e-16 max(1, log K) + 2 u |lse|) + K e^-37

Pinned on oracle/bsc_oracle.py by tests/test_bsc_kernels_cpu.py."""
import itertools

import numpy as np

LD = np.longdouble
NZ_MAX = 16               # PM_BSC_NZ_MAX
NZ_PAD = 0xFFFF
NZ_OVERFLOW = 0xFFFE      # PM_BSC_NZ_OVERFLOW
DEFER_LD = 40             # PM_BSC_DEFER_LD
NSCALARS = 4              # PM_BSC_NSCALARS
NEGLIGIBLE = -37.0
QCUT = -50.0
KEEP_ALL_BELOW = -745.1332191019412       # log(2^-1075): pm_bsc_defer_apply_f64 keeps every datapoint for a cut below it

# pm_bsc_plan: `which`, flags, families, out[] indices
SELECT, ESTEP, MSTEP_ROWS, SELECT_ESTEP, MSTEP_ROWS16, FUSED, FUSED8 = range(7)
F_STATS, F_LISTS = 32, 64
WAVE, LANES16, FAM_FUSED, FAM_FUSED8 = 1, 2, 3, 4
PLAN_LEN = 14
O_FAMILY, O_VPL, O_NJ, O_HP, O_GAMMA, O_FULL, O_MSTATS, O_LDS, O_GRID, O_MAIN_ROWS, O_MAIN_GRID, O_TAIL_ROWS, O_TAIL_GRID, \
    O_TAIL_LDS = range(PLAN_LEN)


# --------------------------------------------------------------------------------------------------------- state tables
def state_matrix(Hp, gamma):
    """(S, H') of generate_state_matrix (camodels/__init__.py:21-47)."""
    rows = []
    for g in range(2, gamma + 1):
        for s in itertools.combinations(range(Hp), g):
            r = np.zeros(Hp, dtype=np.int64)
            r[list(s)] = 1
            rows.append(r)
    return np.array(rows, dtype=np.int64).reshape(len(rows), Hp)


def n_states(Hp, gamma):
    return len(state_matrix(Hp, gamma))


def state_tables(SM, gamma):
    """What the host hands the fast kernels: masks (bit j <=> position j), parents (the state without its highest position;
    0xFFFF when that leaves a singleton), size_offsets (first state of g causes, g = 2 .. gamma; then S)."""
    S, Hp = SM.shape
    masks = (SM << np.arange(Hp)[None, :]).sum(axis=1).astype(np.uint16) if S else np.zeros(0, np.uint16)
    index = {int(m): i for i, m in enumerate(masks)}
    parents = np.full(S, 0xFFFF, dtype=np.uint16)
    for i, m in enumerate(masks.tolist()):
        rest = m & ~(1 << (m.bit_length() - 1))
        if bin(rest).count("1") >= 2:
            parents[i] = index[rest]
    sizes = SM.sum(axis=1)
    off = [int(np.searchsorted(sizes, g, side="left")) for g in range(2, gamma + 1)] + [S]
    off = (off + [S])[:max(gamma, 1)]
    return masks, parents, np.array(off, dtype=np.int32)


def pair_lists(SM):
    """CSR lists of pm_bsc_mstep_rows_f64: the states that contain positions (i, j), for every (i, j)."""
    S, Hp = SM.shape
    ptr, lst = [0], []
    for i in range(Hp):
        for j in range(Hp):
            if S:
                lst.extend(np.nonzero((SM[:, i] == 1) & (SM[:, j] == 1))[0].tolist())
            ptr.append(len(lst))
    return np.array(ptr, dtype=np.int32), np.array(lst, dtype=np.uint16)


# ------------------------------------------------------------------------------------------------------------ selection
def rank_best_last(X, Hp):
    """The H' largest of every row in ascending order (np.argsort(sim)[-H':], bsc_et.py:113); of equal values the larger
    index ranks higher (the documented tie rule: the tail of a stable ascending argsort)."""
    return np.argsort(X, axis=1, kind="stable")[:, -Hp:].astype(np.int64)


def rank_smallest_first(X, Hp):
    """The H' smallest of every row, best first (mode bit 2, mca_et.py:107); of equal values the smaller index first."""
    return np.argsort(X, axis=1, kind="stable")[:, :Hp].astype(np.int64)


def similarity(A, g, yn2=None):
    """sim[n, h] = a / |W_h| (/ |y_n|), bsc_et.py:112, longdouble.  A (N, H) scores, g (H) = |W_h|^2."""
    sim = np.asarray(A, dtype=LD) / np.sqrt(np.asarray(g, dtype=LD))[None, :]
    if yn2 is not None:
        sim = sim / np.sqrt(np.asarray(yn2, dtype=LD))[:, None]
    return sim


def select(A, g, Hp, mode=1, yn2=None):
    """Candidates of pm_bsc_select_f64 (yn2 given) and of the selection pass of the fast kernels (mode bits 2, 3, 4 of
    pm_bsc_select_estep_f64: smallest first | scores as they are | the squared distance |W_h|^2 - 2 a)."""
    A = np.asarray(A, dtype=LD)
    if mode & 16:
        X = np.asarray(g, dtype=LD)[None, :] - 2 * A
    elif mode & 8:
        X = A
    else:
        X = similarity(A, g, yn2)
    return rank_smallest_first(X, Hp) if mode & 4 else rank_best_last(X, Hp)


# --------------------------------------------------------------------------------------------------------------- E-step
def energies(Y, Wt, mu, cand, SM):
    """|y - mu - sum_h s_h W_h|^2 of every column's state (bsc_et.py:170-182), longdouble: (N, 1 + H + S)."""
    Y, Wt = np.asarray(Y, dtype=LD), np.asarray(Wt, dtype=LD)
    N, H, S = Y.shape[0], Wt.shape[0], SM.shape[0]
    y = Y if mu is None else Y - np.asarray(mu, dtype=LD)[None, :]
    E = np.empty((N, 1 + H + S), dtype=LD)
    E[:, 0] = (y * y).sum(axis=1)
    for n in range(N):
        E[n, 1:1 + H] = ((Wt - y[n]) ** 2).sum(axis=1)
        if S:
            Wbar = SM.astype(LD) @ Wt[np.asarray(cand[n], dtype=np.int64)]
            E[n, 1 + H:] = ((Wbar - y[n]) ** 2).sum(axis=1)
    return E


def state_sizes(H, SM):
    return np.concatenate([[0], np.ones(H, dtype=np.int64), SM.sum(axis=1)]).astype(np.int64)


def log_joints(E, sizes, pil_bar, ecoef, prior_scale):
    """prior_scale pil_bar |s| + ecoef e (bsc_et.py:187-190 with ecoef = beta pre1), longdouble."""
    return LD(prior_scale) * LD(pil_bar) * np.asarray(sizes, dtype=LD)[None, :] + LD(ecoef) * np.asarray(E, dtype=LD)


def lse(F):
    F = np.asarray(F, dtype=LD)
    m = F.max(axis=1)
    return m + np.log(np.exp(F - m[:, None]).sum(axis=1))


def lse_bound(K, lanes, l):
    """|lse_kernel - lse| allowed (derivation: module docstring)."""
    u = 2.0 ** -53
    steps = -(-K // lanes) + int(np.log2(lanes))
    rounding = steps * (4.6e-16 + 2 * u) + 2e-16 * max(1.0, np.log(K)) + 2 * u * np.abs(l)
    return 4 * rounding + K * np.exp(NEGLIGIBLE)


def dropped(F64, against, cut):
    """Columns with F64 - against[n] > cut false, in float64 as the kernels evaluate it."""
    with np.errstate(invalid="ignore"):
        return ~(np.asarray(F64, dtype=np.float64) - np.asarray(against, dtype=np.float64)[:, None] > cut)


def dropped_onepass(F64):
    """... of the one-pass kernels: f > max + NEGLIGIBLE false (the sum is formed first there, exactly)."""
    F64 = np.asarray(F64, dtype=np.float64)
    return ~(F64 > (F64.max(axis=1) + NEGLIGIBLE)[:, None])


# --------------------------------------------------------------------------------------------------------------- M-step
def stats_len(H, D):
    return H * D + H * H + 2 * H + NSCALARS


def stats_sections(H, D):
    o = H * D
    return dict(Wp=slice(0, o), Wq=slice(o, o + H * H), qdiag=slice(o + H * H, o + H * H + H),
                mus=slice(o + H * H + H, o + H * H + 2 * H), scalars=slice(o + H * H + 2 * H, o + H * H + 2 * H + NSCALARS))


def pair_entry(i, k):
    """Entry of positions i <= k in a deferred record."""
    return k * (k + 1) // 2 + i


def row_stats(F, l, keep, E, cand, SM, H, ecoef, mult=None, drop=None):
    """The per-datapoint part of the M-step (bsc_et.py:271-272, 334-366, 395-415) for the rows with keep[n]: posterior
    weights q = exp(F - l).  mult[n]: how many datapoints are copies of row n.  drop (N, K) bool: weights that count as zero.

    Returns a dict (longdouble):  expect (N, H): E[s] rows, zero where not kept;  q1 (H), m1 (H): column sums of the
    singletons' weights and of the multi-cause states' share of E[s];  upper (H, H): the strict upper triangle of
    sum_n E[s s^T] over the multi-cause states (pair (a, b) of positions at (min, max) of its latents);  sig = sum q e,
    fs = sum lse, cnt;  records (N, DEFER_LD): [pair entries k (k + 1) / 2 + i, i < k; the diagonal entries zero | ecoef sum_k
    q_k e_k | zeros], of every row, kept or not;  nz_cnt (N): non-zeros of the E[s] rows as if every row were kept."""
    F, E = np.asarray(F, dtype=LD), np.asarray(E, dtype=LD)
    N, K = F.shape
    S, Hp = SM.shape
    SMl = SM.astype(LD)
    mult = np.ones(N, dtype=np.int64) if mult is None else np.asarray(mult)
    expect = np.zeros((N, H), dtype=LD)
    full = np.zeros((N, H), dtype=LD)
    q1, m1, upper = np.zeros(H, dtype=LD), np.zeros(H, dtype=LD), np.zeros((H, H), dtype=LD)
    records = np.zeros((N, DEFER_LD), dtype=LD)
    sig = fs = cnt = LD(0)
    for n in range(N):
        q = np.exp(F[n] - LD(l[n]))
        if drop is not None:
            q = np.where(drop[n], LD(0), q)
        qs = q[1 + H:]
        cn = np.asarray(cand[n], dtype=np.int64)
        m = qs @ SMl if S else np.zeros(Hp, dtype=LD)              # (H',): the states' share of E[s] per position
        B = (SMl * qs[:, None]).T @ SMl if S else np.zeros((Hp, Hp), dtype=LD)
        full[n] = q[1:1 + H]
        full[n, cn] += m
        for a in range(Hp):
            for b in range(a + 1, Hp):
                records[n, pair_entry(a, b)] = B[a, b]
        records[n, 36] = LD(ecoef) * (q * E[n]).sum()
        if not keep[n]:
            continue
        w = LD(int(mult[n]))
        expect[n] = full[n]
        q1 += w * q[1:1 + H]
        m1[cn] += w * m
        for a in range(Hp):
            for b in range(a + 1, Hp):
                upper[min(cn[a], cn[b]), max(cn[a], cn[b])] += w * B[a, b]
        sig += w * (q * E[n]).sum()
        fs += w * LD(l[n])
        cnt += w
    return dict(expect=expect, q1=q1, m1=m1, upper=upper, sig=sig, fs=fs, cnt=cnt, records=records,
                nz_cnt=(full != 0).sum(axis=1))


def pack_stats(st, H, D, convention, overflow=0):
    """The packed buffer [Wp | Wq | qdiag | mus | scalars] a call adds to, longdouble, and the mask of entries it may write.
    convention: "rows" (pm_bsc_mstep_rows_f64, _rows16_f64), "fused" (pm_bsc_estep_fused_f64), "fused8" (the whole-shard
    passes and pm_bsc_defer_apply_f64)."""
    out = np.zeros(stats_len(H, D), dtype=LD)
    sec = stats_sections(H, D)
    Wq = st["upper"].copy()
    mus = st["q1"] + st["m1"]
    if convention in ("rows", "fused"):
        Wq[np.arange(H), np.arange(H)] = st["m1"]
    out[sec["Wq"]] = Wq.reshape(-1)
    if convention == "rows":
        out[sec["qdiag"]] = st["q1"]
    elif convention == "fused8":
        out[sec["qdiag"]] = mus
    out[sec["mus"]] = mus
    out[sec["scalars"]] = [st["sig"], st["fs"], st["cnt"], overflow]
    return out


def lists_of(expect, keep=None):
    """nz_idx (N, NZ_MAX) of E[s] rows: the ascending non-zero latents, the first NZ_MAX kept, the other slots NZ_PAD; and
    the non-zero counts."""
    expect = np.asarray(expect)
    N = expect.shape[0]
    idx = np.full((N, NZ_MAX), NZ_PAD, dtype=np.int64)
    cnt = np.zeros(N, dtype=np.int64)
    for n in range(N):
        nz = np.nonzero(expect[n] != 0)[0]
        cnt[n] = len(nz)
        idx[n, :min(len(nz), NZ_MAX)] = nz[:NZ_MAX]
    return idx, cnt


# ------------------------------------------------------------------------------------------------------ sparse products
def expand_lists(idx, val, H, into):
    """pm_bsc_expand_lists_gated_f64 with an open gate: rows whose slot 0 is not NZ_OVERFLOW become their list."""
    out = np.array(into, dtype=np.float64, copy=True)
    for n in range(idx.shape[0]):
        if idx[n, 0] == NZ_OVERFLOW:
            continue
        out[n, :H] = 0.0
        for t in range(NZ_MAX):
            if idx[n, t] != NZ_PAD:
                out[n, idx[n, t]] = val[n, t]
    return out


def wp_sparse(idx, val, Y, H):
    """sum_n sum_t val[n, t] Y[n, :] into row idx[n, t] (my_Wp of bsc_et.py:339-363 from the lists): (H, D) longdouble.
    Slots holding NZ_PAD or NZ_OVERFLOW carry nothing."""
    Y = np.asarray(Y, dtype=LD)
    Wp = np.zeros((H, Y.shape[1]), dtype=LD)
    for n in range(idx.shape[0]):
        for t in range(NZ_MAX):
            if idx[n, t] < H:
                Wp[idx[n, t]] += LD(val[n, t]) * Y[n]
    return Wp


# ---------------------------------------------------------------------------------------------------------------------
# The shapes and data of tests/test_bsc_kernels_gpu.py (tests/test_bsc_kernels_cpu.py pins the plan of every shape, the
# exactness of its arithmetic and the spread of its posterior weights without a device).
# ---------------------------------------------------------------------------------------------------------------------
PERIOD = 67          # rows of a main-launch case repeat with this period (prime: no multiple of a tile or of a pass of four)
RING_K = 32          # K columns the four-stage ring of the fused kernels holds (STAGES = 4 stages x DK = 8 columns)


def case_N(spec, cus):
    """Datapoints of a case: a literal, or a rule in the device's compute units."""
    if isinstance(spec, int):
        return spec
    return {"main": 2 * cus * 16 + 1, "both": cus * 128 + 17}[spec]


def _fused8_cases():
    """One case per instantiation <HP, GAMMA, FULL, MSTATS, TAIL> of bsc_estep_fused8s_kernel: 64.  H, N and D walk through
    the values the kernel's edges sit at (TAIL: N in {1, 15, 16, 17, 33}, D in {8, 16, 32, 40} -- the K split four ways, three
    slices empty at D = 8; main: D in {8, the ring depth, one stage more})."""
    cases = {}
    tn, td, md = [1, 15, 16, 17, 33], [8, 16, 32, 40], [8, RING_K, RING_K + 8]
    i = j = 0
    for tail in (1, 0):
        for hp in (5, 6, 7, 8):
            for g in (3, 4):
                for full in (0, 1):
                    for ms in (0, 1):
                        H = 256 if full else ((129, 200) if tail else (129, 255))[j % 2]
                        j += 0 if full else 1
                        N = tn[i % 5] if tail else "main"
                        D = td[(i // 3) % 4] if tail else md[i % 3]
                        name = "%s_hp%d_g%d_%s_%s" % ("tail" if tail else "main", hp, g, "full" if full else "part",
                                                      "ms" if ms else "e")
                        cases[name] = dict(entry="fused8", H=H, Hp=hp, gamma=g, D=D, N=N, stats=bool(ms), mu=False,
                                           cell=(hp, g, full, ms, tail))
                        i += 1
    cases["main_hp8_g4_full_ms_mu"] = dict(entry="fused8", H=256, Hp=8, gamma=4, D=RING_K, N="main", stats=True, mu=True,
                                           cell=(8, 4, 1, 1, 0))
    cases["tail_hp6_g3_part_ms_mu"] = dict(entry="fused8", H=200, Hp=6, gamma=3, D=16, N=33, stats=True, mu=True,
                                           cell=(6, 3, 0, 1, 1))
    cases["both_hp7_g3_part_ms"] = dict(entry="fused8", H=255, Hp=7, gamma=3, D=16, N="both", stats=True, mu=False,
                                        cell=(7, 3, 0, 1, 2))
    return cases


def _vpl16(H):
    return 1 if H <= 16 else 2 if H <= 32 else 4 if H <= 64 else 8 if H <= 128 else 16 if H <= 256 else 32


def _other_cases():
    """The cells of the other launchers: `cell` is what pm_bsc_plan must report for the case (family, VPL or NJ, ...).
    select: one H on each side of every VPL switch of bsc_select_kernel.  wave: the generic kernels, with S = 0 and mu.
    select_estep / rows16: H at every VPL boundary of the sixteen-lane kernels and one past it (H = 16 and 17 run hot with
    exactly PM_BSC_NZ_MAX non-zeros per row and one more).  fused: NJ 8 and 16, FULL and not, with and without statistics, N
    on both sides of the 64-row tile, D one K-step short of the ring, the ring, one more."""
    cases = {}
    for H in (64, 65, 128, 129, 256, 257, 512, 513):
        cases["sel_h%d" % H] = dict(entry="select", H=H, Hp=6, gamma=1, D=8, N=5, stats=False, mu=False,
                                    cell=(WAVE, 1 if H <= 64 else 2 if H <= 128 else 4 if H <= 256 else 8 if H <= 512 else 16))
    for (H, Hp, g), N in zip(((5, 3, 2), (12, 5, 3), (70, 6, 3)), (1, 4, 5)):
        cases["wave_h%d" % H] = dict(entry="wave", H=H, Hp=Hp, gamma=g, D=8, N=N, stats=True, mu=(H == 12), cell=(WAVE,))
    cases["wave_s0"] = dict(entry="wave", H=12, Hp=5, gamma=1, D=8, N=5, stats=True, mu=False, cell=(WAVE,))
    Ns = [1, 15, 16, 17, 65]
    for i, H in enumerate((16, 17, 32, 33, 64, 65, 128, 129, 256, 257)):
        cases["se_h%d" % H] = dict(entry="select_estep", H=H, Hp=5, gamma=(3, 5, 1)[i % 3], D=8, N=Ns[i % 5], stats=False,
                                   mu=(i % 4 == 1), cell=(LANES16, _vpl16(H)))
    for H in (16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512):
        cases["r16_h%d" % H] = dict(entry="rows16", H=H, Hp=5, gamma=3, D=8, N=17, stats=True, mu=False,
                                    cell=(LANES16, _vpl16(H)))
    Nf, Df = [1, 63, 64, 65, 129], [8, RING_K - 8, RING_K, RING_K + 8]
    i = 0
    for H in (16, 128, 129, 256):
        for st in (0, 1):
            cases["fused_h%d_%s" % (H, "ms" if st else "e")] = dict(
                entry="fused", H=H, Hp=5, gamma=3, D=Df[i % 4], N=Nf[i % 5], stats=bool(st), mu=(i == 3),
                cell=(FAM_FUSED, 8 if H <= 128 else 16, 1 if H in (128, 256) else 0, st))
            i += 1
    return cases


CASES = _fused8_cases()
# the cases the list-writing entries run on: TAIL and main launches, mu; cold, they hold a row with exactly NZ_MAX non-zeros
# (tail_hp6_g4_part_ms) and rows with NZ_MAX + 1 (the other two without mu)
LIST_CASES = ["tail_hp6_g4_part_ms", "tail_hp6_g3_part_ms", "tail_hp6_g3_part_ms_mu", "main_hp8_g4_full_ms"]
CASES.update(_other_cases())


def weights(H, D, seed):
    """Wt (H, D): every row has |W_h|^2 a power of 4 (one entry +-1, +-2 or +-4; four entries +-1 or +-2 where D >= 4), and
    every row pattern occurs two or three times at distant latents -- those latents tie in any arithmetic."""
    rng = np.random.RandomState(seed)
    distinct = -(-H * 2 // 5)
    base = np.zeros((distinct, D))
    for r in range(distinct):
        kind = (r + seed) % 5
        if kind < 3:
            base[r, rng.randint(D)] = [1.0, 2.0, 4.0][kind] * rng.choice([-1.0, 1.0])
        else:
            pos = rng.permutation(D)[:4]
            base[r, pos] = [1.0, 2.0][kind - 3] * rng.choice([-1.0, 1.0], size=4)
    owner = np.concatenate([np.arange(distinct), np.arange(distinct), np.arange(0, distinct, 2)])[:H]
    assert len(owner) == H
    return base[(owner * 7 + seed) % distinct]


def ints(rows, cols, seed, lo=-8, hi=8):
    """Position-dependent integers in [lo, hi] as f64."""
    rng = np.random.RandomState(seed)
    i, j = np.arange(rows)[:, None], np.arange(cols)[None, :]
    return (lo + (rng.randint(0, hi - lo + 1, size=(rows, cols)) + (i + 3 * j) % 5) % (hi - lo + 1)).astype(np.float64)


def make_case(name, hot, cus=256, seed=0):
    """The operands of a case as a dict.  Y, Wt and mu are small integers, so scores, Gram entries, |y|^2, W mu, Y mu and |mu|^2
    are exact in any summation order; |W_h|^2 is a power of 4, so the ranking key a / |W_h| is exact; ecoef is -2^-20 (hot:
    with pil_bar = -1/16 all weights of a row lie within a factor e) or -2 (cold: pil_bar = -9/16, prior_scale = 1/2; terms
    below the kernels' cut-offs occur)."""
    spec = CASES[name]
    H, Hp, gamma, D = spec["H"], spec["Hp"], spec["gamma"], spec["D"]
    N = case_N(spec["N"], cus)
    sd = seed + 1000 * (sum(map(ord, name)) % 97)
    rows = min(N, PERIOD) if N > 1000 else N
    Wt = weights(H, D, sd + 1)
    Y = ints(rows, D, sd + 2, -6, 6)
    # row 0 ties at the H' boundary (the case may have no other row): the first of a fixed sequence of rows that does
    root = np.sqrt((Wt * Wt).sum(axis=1))
    for k in range(1024):
        y0 = ints(1, D, sd + 7 + k, -6, 6)[0]
        y0 = np.where(y0 == 0, 1.0, y0)
        srt = np.sort((Wt @ y0) / root)
        if srt[-Hp] == srt[-Hp - 1] and (srt[-Hp] != srt[-1] or k >= 256):
            break
    else:
        raise AssertionError("no row with a tie at the H' boundary: " + name)
    Y[0, :] = y0
    mu =ints(1, D, sd + 3, -2, 2)[0] if spec["mu"] else None
    SM = state_matrix(Hp, gamma)
    masks, parents, size_off = state_tables(SM, gamma)
    if hot:
        ecoef, prior_scale, pil_bar = -2.0 ** -20, 1.0, -1.0 / 16
    else:
        ecoef, prior_scale, pil_bar = -2.0, 0.5, -9.0 / 16
    A = Y @ Wt.T
    G = Wt @ Wt.T
    rep = -(-N // rows)
    t = (lambda x: np.tile(x, (rep,) + (1,) * (x.ndim - 1))[:N])
    c = dict(spec, name=name, hot=hot, N=N, rows=rows, S=len(SM), K=1 + H + len(SM), Y=t(Y), Wt=Wt, mu=mu, SM=SM, masks=masks,
             parents=parents, size_off=size_off, A=t(A), G=G, yn2=t((Y * Y).sum(axis=1)), ecoef=ecoef, prior_scale=prior_scale,
             pil_bar=pil_bar, wmu=None if mu is None else Wt @ mu, ymu=None if mu is None else t(Y @ mu),
             mu_sqnorm=0.0 if mu is None else float(mu @ mu))
    # candidates handed in under mode 2 (not the selected ones: distinct latents in a position-dependent order)
    rng = np.random.RandomState(sd + 5)
    c["cand_in"] = t(np.stack([rng.permutation(H)[:Hp] for _ in range(rows)]).astype(np.int32))
    return c


def mult(c):
    """Datapoints per distinct row of a (periodic) case."""
    return np.bincount(np.arange(c["N"]) % c["rows"], minlength=c["rows"])


def tile(c, x):
    rep = -(-c["N"] // c["rows"])
    return np.tile(x, (rep,) + (1,) * (x.ndim - 1))[:c["N"]]


def case_reference(c, cand=None):
    """Candidates (selected, unless given), energies, log-joints (longdouble and, exactly, float64) and lse of the distinct
    rows of a case; ``exact``: what the equality comparisons rest on (tests/test_bsc_kernels_cpu.py)."""
    r, H, Hp = c["rows"], c["H"], c["Hp"]
    g = np.diag(c["G"])
    if cand is None:
        cand = select(c["A"][:r], g, Hp)
    else:
        cand = np.asarray(cand[:r], dtype=np.int64)
    key = c["A"][:r] / np.sqrt(g)[None, :]                                       # float64: the kernels' ranking key
    srt = np.sort(key, axis=1)
    E = energies(c["Y"][:r], c["Wt"], c["mu"], cand, c["SM"])
    sizes = state_sizes(H, c["SM"])
    F = log_joints(E, sizes, c["pil_bar"], c["ecoef"], c["prior_scale"])
    F64 = (c["prior_scale"] * c["pil_bar"]) * sizes[None, :].astype(np.float64) + c["ecoef"] * E.astype(np.float64)
    root = np.sqrt(g)
    exact = bool(
        (E == np.rint(E)).all() and np.abs(E).max() < 2.0 ** 30 and (F64.astype(LD) == F).all()
        and (root == np.rint(root)).all() and (np.log2(root) == np.rint(np.log2(root))).all()      # |W_h| a power of two
        and (key.astype(LD) == similarity(c["A"][:r], g)).all()
        and (np.abs(key) * 2.0 ** 10 == np.rint(np.abs(key) * 2.0 ** 10)).all() and np.abs(key).max() < 2.0 ** 20)
    return dict(cand=cand, E=E, F=F, F64=F64, lse=lse(F), exact=exact,
                boundary_ties=int((srt[:, -Hp] == srt[:, -Hp - 1]).sum()))
