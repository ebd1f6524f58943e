"""Plain NumPy (longdouble) restatement of the exact top-K entries (include/prosper_hip.h: pm_infer_exact_*) on
the KERNELS' operands, built on ``_lin_logjoint`` / ``_mca_logjoint`` of tests/exact_kernels_reference.py.  Shared by
tests/test_infer_exact_cpu.py (which pins it) and the GPU modules tests/test_infer_exact_abi_gpu.py and
tests/test_infer_exact_gpu.py.  Not a test module.

  topk_rows      the top-K of every row of a log-joint table under the order (larger value, then smaller state index), v_n
                 and the NaN convention of the entries;
  assert_margin  the condition under which rounding cannot swap neighbours: in the reference's own values, consecutive
                 entries among a row's topK + 1 best differ by more than MARGIN max(1, |l|) -- asserted for EVERY row of a case;
  lin_top / mca_top   (idx, l, v) of the two entries from their operands;
  infer_plan     pm_infer_exact_plan restated from the header's prose;
  planted_lin / planted_mca   operands whose log-joints are exact small integers, and the expected order;
  the case tables the GPU module runs and the CPU module pins to the plan.
"""
import numpy as np

import exact_kernels_reference as R

LD = np.longdouble
PM_OK, PM_EINVAL, PM_ERANGE = R.PM_OK, R.PM_EINVAL, R.PM_ERANGE
LIN, MCA, GSC = R.LIN, R.MCA, R.GSC
PLAN_LEN = 12
MAX_TOPK = 16
MARGIN = 1e-9


def topk_rows(l, topK):
    """(idx (N, cols) int64, vals (N, cols) longdouble, v (N,) longdouble), cols = min(topK, S): a stable sort of -l, so that
    equal values keep their index order and -inf comes last by index.  A row with a NaN: idx -1, NaN values, NaN v."""
    l = np.asarray(l, dtype=LD)
    N, S = l.shape
    cols = min(int(topK), S)
    bad = np.isnan(l).any(axis=1)
    safe = np.where(bad[:, None], LD(0), l)
    with np.errstate(invalid="ignore"):
        order = np.argsort(-safe, axis=1, kind="stable")[:, :cols].astype(np.int64)
    vals = np.take_along_axis(safe, order, axis=1)
    v = R.lse_rows(l)[0]
    order[bad] = -1
    vals[bad] = LD("nan")
    return order, vals, v


def margin(l, topK):
    """The smallest relative gap, over all rows, between consecutive entries among the topK + 1 best (pairs of -inf, which
    tie exactly in every arithmetic and are ordered by index alone, are left out)."""
    l = np.asarray(l, dtype=LD)
    _, vals, _ = topk_rows(l, min(int(topK) + 1, l.shape[1]))
    worst = np.inf
    for row in vals:
        for a, b in zip(row[:-1], row[1:]):
            if a == -np.inf and b == -np.inf:
                continue
            if b == -np.inf:
                continue                                         # finite above -inf: an infinite gap
            worst = min(worst, float((a - b) / max(LD(1), abs(a), abs(b))))
    return worst


def assert_margin(l, topK):
    g = margin(l, topK)
    assert g > MARGIN, "a near-tie among the topK + 1 best (relative gap %.3e): choose another seed" % g
    return g


def lin_table(Y, ymu, P, G, logp, values):
    B, _ = R.lin_prep(Y, ymu, P)
    return R._lin_logjoint(B, G, logp, values)[0]


def mca_table(Y, Wrho, inv_rho, signed, lp1, lp0, inv_s2):
    return R._mca_logjoint(Y, Wrho, inv_rho, signed, lp1, lp0, inv_s2)[0]


def lin_top(Y, ymu, P, G, logp, values, topK, check=True):
    l = lin_table(Y, ymu, P, G, logp, values)
    if check:
        assert_margin(l, topK)
    return topk_rows(l, topK)


def mca_top(Y, Wrho, inv_rho, signed, lp1, lp0, inv_s2, topK, check=True):
    l = mca_table(Y, Wrho, inv_rho, signed, lp1, lp0, inv_s2)
    if check:
        assert_margin(l, topK)
    return topk_rows(l, topK)


# ------------------------------------------------------------------------------------------------------------------ plan
def infer_plan(kind, N, D, K, H, topK):
    """pm_infer_exact_plan: (code, out) from the header's description."""
    if N < 0 or D < 1 or H < 1 or topK < 1:
        return PM_EINVAL, None
    if kind == LIN:
        if not 2 <= K <= 8:
            return PM_EINVAL, None
        if H > 32 or K ** H > 2 ** 32:
            return PM_ERANGE, None
        L, CH = R.lin_split(K, H)
        states, space, rows, boff = K ** H, K ** (H - L), 256, H
        Rr = min(256, max(1, space // 2))
    elif kind == MCA:
        if H > 32 or D > 1024:
            return PM_ERANGE, None
        L, CH, states, space, rows, boff = 0, 1, 2 ** H, 2 ** H, 64, 0
        Rr = min(64, max(1, space // 64))
    else:
        return PM_EINVAL, None
    if topK > MAX_TOPK:
        return PM_ERANGE, None
    cols = min(topK, states)
    nb = min(N, rows)
    o_lse, n_lse, n_list = nb * boff, 2 * nb * Rr, nb * Rr * cols
    return PM_OK, [rows, -(-N // rows), L, CH, space, Rr, cols, o_lse, n_lse, o_lse + n_lse, o_lse + n_lse + n_list, n_list]


def work_len(N, H, topK):
    if N < 0 or H < 1 or topK < 1 or topK > MAX_TOPK:
        return -1
    return max(min(N, 256) * (H + 256 * (2 + 2 * topK)), min(N, 64) * 64 * (2 + 2 * topK), 1)


def state_cell(kind, K, H, topK):
    """The cell of a call's walk over the states: what separates one path through the sweep and the merges from another."""
    rc, p = infer_plan(kind, 3, 5, K, H, topK)
    assert rc == PM_OK
    L, CH, space, Rr, cols = p[2:7]
    per = -(-space // Rr)                              # units of the longest range
    return (kind, "cols<topK" if cols < topK else "cols=topK", "R=1" if Rr == 1 else "R=2" if Rr == 2 else "R>2",
            "states" if kind == MCA else "one chunk" if space == 1 else "two chunks" if per == 2 else "chunks",
            "ragged lo" if kind == LIN and CH % 256 else "full lo")


def walk_cell(kind, N):
    """... and of the host walk over the row blocks."""
    rows = 256 if kind == LIN else 64
    return (kind, "short block" if N < rows else "full block" if N == rows else "blocks")


# ------------------------------------------------------------------------------------------------------ planted operands
def planted_lin(K, H, t, D=3):
    """Operands with Y = ymu and G = 0: l(s) = sum_h logp[h, k_h] = -(Hamming distance of s to the state with index t),
    exact in every arithmetic.  Returns (operands, dist (S,) int64)."""
    dig = (t // K ** np.arange(H)) % K
    logp = -np.ones((H, K))
    logp[np.arange(H), dig] = 0.0
    ymu = np.linspace(-1.0, 1.0, D)
    ops = dict(ymu=ymu, P=np.ones((D, H)) * 0.5, G=np.zeros((H, H)), logp=logp, values=np.arange(K, dtype=np.float64), K=K)
    idx = np.arange(K ** H, dtype=np.int64)
    sd = (idx[:, None] // (K ** np.arange(H, dtype=np.int64))[None, :]) % K
    return ops, (sd != dig[None, :]).sum(axis=1)


def planted_order(score, topK):
    """The first topK state indices by (smaller score, smaller index) and their scores."""
    order = np.argsort(score, kind="stable")[:topK]
    return order.astype(np.int64), score[order]


def popcounts(H):
    idx = np.arange(1 << H, dtype=np.int64)
    return ((idx[:, None] >> np.arange(H, dtype=np.int64)[None, :]) & 1).sum(axis=1)


# ------------------------------------------------------------------------------------------------------------- case tables
# Random cases of the linear entry: (K, H, N, topK, seed).  K = 2: H = 1 and 3 hold fewer states than topK; H = 10 is one
# chunk; H = 11 two chunks in one range; H = 12 the first two-range merge; H = 14 eight ranges.  K = 3: H = 7 (729 of 768 lo
# slots, 3 chunks, R = 1) and H = 8 (R = 4).  K = 8, H = 4: 512 lo states, 8 chunks, R = 4.  N walks the 256-row blocks at H = 12.
LIN_CASES = [
    (2, 1, 3, 10, 0), (2, 3, 3, 10, 0), (2, 3, 3, 2, 0), (2, 3, 2, MAX_TOPK, 1), (2, 10, 3, 10, 0), (2, 11, 3, 10, 0), (2, 12, 1, 10, 0),
    (2, 12, 255, 1, 1), (2, 12, 256, 2, 2), (2, 12, 257, 10, 0), (2, 14, 2, MAX_TOPK, 0),
    (3, 7, 3, 10, 0), (3, 8, 2, MAX_TOPK, 0), (8, 4, 2, 10, 0), (2, 13, 2, 2, 1),
]
# ... of the MCA entry: (signed, H, N, D, topK, seed): the cells MCA_RECON_* of tests/exact_kernels_reference.py name
MCA_CASES = [
    (0, 1, 63, 5, 10, 0), (1, 6, 64, 63, 10, 0), (0, 6, 65, 64, 1, 1), (1, 6, 3, 65, 2, 2), (0, 6, 3, 128, MAX_TOPK, 0),
    (0, 11, 3, 1, 10, 0), (1, 11, 65, 7, MAX_TOPK, 1), (0, 10, 2, 9, 10, 2), (0, 7, 2, 4, 10, 0),
]
# The grid the CPU module sweeps for cells: every cell it finds must be the cell of a case above.
CELL_GRID_LIN = [(K, H) for K, Hs in ((2, (1, 3, 10, 11, 12, 13, 14)), (3, (7, 8)), (8, (4,))) for H in Hs]
CELL_GRID_MCA = (1, 6, 7, 10, 11)
CELL_TOPK = (1, 2, 10, MAX_TOPK)
CELL_N = {LIN: R.LIN_RECON_N, MCA: R.MCA_RECON_N}
