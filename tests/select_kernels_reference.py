"""Plain statements of what infer_kernels.hip, kth_select.hip and spd_inverse.hip compute -- nothing of lanes, tiles or rounds
of a wavefront: Python's ``sorted`` for the ranking, longdouble for every log-sum-exp, Python integers for the radix select's
keys, ``fractions.Fraction`` for the exact inverse.  Pinned by tests/test_select_kernels_cpu.py, used by
tests/test_select_kernels_gpu.py."""
from fractions import Fraction

import numpy as np

LD = np.longdouble
GAP = 64.0                      # K exp(-GAP) < 2^-54 up to K = 4000: such a row's log-sum-exp IS its maximum, bit for bit
KTH_ROUNDS = ((52, 12), (40, 12), (28, 12), (16, 12), (4, 12), (0, 4))
BINS = 4096


# ------------------------------------------------------------------------------------------------------------- top-K
def lse(values):
    """log sum exp in longdouble, the maximum taken over the comparable (non-NaN) entries; NaN / inf as they fall out."""
    v = np.asarray(values, dtype=LD)
    comp = v[~np.isnan(v)]
    m = comp.max() if comp.size else LD(-np.inf)
    with np.errstate(all="ignore"):
        return m + np.log(np.exp(v - m).sum()), m


def ranking(row):
    """Columns descending by (value, column), NaN entries skipped."""
    return [k for _, k in sorted(((float(v), k) for k, v in enumerate(row) if v == v), reverse=True)]


def _ranked(row, order, topK, l, m):
    idx = np.full(topK, -1, dtype=np.int32)
    lpc, rel = np.full(topK, -np.inf, dtype=LD), np.full(topK, -np.inf)
    with np.errstate(all="ignore"):
        for r, k in enumerate(order[:topK]):
            idx[r], lpc[r], rel[r] = k, LD(row[k]) - l, row[k] - np.float64(m)       # (v - max: one float64 operation)
    return idx, lpc, rel


def topk(F, cand, masks, H, single_cols, topK):
    """F (N, K = 1 + single_cols + S), cand (N, Hp) distinct latents, masks (S,) uint16.  Returns top_idx (int32), top_lpc
    (longdouble), top_rel (float64: v - max is one correctly rounded operation), marg (N, H) longdouble, lse (N,) and
    marg_single (N, H) bool: a candidate's marginal all of whose terms but the largest are -inf or at least GAP below it."""
    F = np.asarray(F, dtype=np.float64)
    N, K = F.shape
    S, moff, Hp = K - 1 - single_cols, 1 + single_cols, cand.shape[1]
    out = dict(top_idx=np.empty((N, topK), np.int32), top_lpc=np.empty((N, topK), LD), top_rel=np.empty((N, topK)),
               marg=np.empty((N, H), LD), lse=np.empty(N, LD), marg_single=np.zeros((N, H), bool))
    with np.errstate(all="ignore"):
        for n in range(N):
            row = F[n]
            l, m = lse(row)
            out["lse"][n] = l
            out["top_idx"][n], out["top_lpc"][n], out["top_rel"][n] = _ranked(row, ranking(row), topK, l, m)
            out["marg"][n] = row[1:1 + H].astype(LD) - l
            for j in range(Hp):
                c = int(cand[n, j])
                terms = np.asarray([row[1 + c]] + [row[moff + s] for s in range(S) if (int(masks[s]) >> j) & 1], dtype=np.float64)
                lt, mt = lse(terms)
                out["marg"][n, c] = LD(-np.inf) if mt == -np.inf else lt - l
                others = np.sort(terms)[:-1]
                out["marg_single"][n, c] = bool(np.isfinite(mt) and (others <= mt - GAP).all())
    return out


def topk_signed(F, cand, vals, H, topK, rank, top_idx_in=None):
    """F (N, S), cand (N, Hp) latents (repeats allowed), vals (S, Hp) in {-1, 0, 1}.  Returns top_idx, tie (rank != 0), top_lpc,
    top_post (longdouble), and the writes: s (N, topK, H) int8 with s_written, m / am (N, H) longdouble with m_written -- an
    entry that is not written is left as it was."""
    F = np.asarray(F, dtype=np.float64)
    N, S = F.shape
    Hp = cand.shape[1]
    out = dict(top_idx=np.empty((N, topK), np.int32), tie=np.zeros(N, np.int32), top_lpc=np.empty((N, topK), LD),
               top_post=np.empty((N, topK), LD), lse=np.empty(N, LD), s=np.zeros((N, topK, H), np.int8),
               s_written=np.zeros((N, topK, H), bool), m=np.zeros((N, H), LD), am=np.zeros((N, H), LD),
               m_written=np.zeros((N, H), bool), am_mag=np.zeros((N, H), LD))
    with np.errstate(all="ignore"):
        for n in range(N):
            row = F[n]
            l, _ = lse(row)
            l64 = np.float64(l)
            out["lse"][n] = l
            if rank:
                order = ranking(row)
                idx = np.full(topK, -1, dtype=np.int32)
                idx[:min(topK, len(order))] = order[:topK]
                best = [row[k] for k in order[:min(topK + 1, S)]]
                out["tie"][n] = int(any(a == b or (a - l64) == (b - l64) for a, b in zip(best, best[1:])))
            else:
                idx = np.asarray(top_idx_in[n], dtype=np.int32)
            out["top_idx"][n] = idx
            p = np.exp(row.astype(LD) - l)
            for r, k in enumerate(idx):
                ok = 0 <= k < S
                out["top_lpc"][n, r] = LD(row[k]) - l if ok else LD(-np.inf)
                out["top_post"][n, r] = np.exp(LD(row[k]) - l) if ok else LD(0)
                if ok:
                    for j in range(Hp):
                        out["s"][n, r, cand[n, j]] = vals[k, j]
                        out["s_written"][n, r, cand[n, j]] = True
            for j in range(Hp):
                c = int(cand[n, j])
                out["m"][n, c] = (p * vals[:, j]).sum()
                out["am"][n, c] = out["am_mag"][n, c] = (p * np.abs(vals[:, j])).sum()
                out["m_written"][n, c] = True
    return out


# ------------------------------------------------------------------------------------------------------ k-th largest
def key_of_int(bits):
    """The header's order-preserving key of a double given by its 64 bits, as a Python int: larger double <=> larger key."""
    b = int(bits)
    return (~b) & 0xFFFFFFFFFFFFFFFF if b >> 63 else b | (1 << 63)


def bits_of_key(k):
    k = int(k)
    return k & 0x7FFFFFFFFFFFFFFF if k >> 63 else (~k) & 0xFFFFFFFFFFFFFFFF


def keys_of(x):
    """key_of_int of every element of a float64 array (uint64)."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | np.uint64(1 << 63))


def doubles_of_keys(keys):
    k = np.asarray(keys, dtype=np.uint64)
    return np.where(k >> np.uint64(63) != 0, k & np.uint64(0x7FFFFFFFFFFFFFFF), ~k).astype(np.uint64).view(np.float64)


def kth(keys_by_shard, k):
    """The k-th largest (1-based) of the shards' keys.  Returns (value bits as uint64, states (7, 2), hists (6, 4096)):
    round r counts, per digit of [shift, shift + bits), the keys that agree with the prefix above the digit; the digit taken is the
    highest d with count(digits >= d) >= k (0 if none), and k becomes k - count(digits > d)."""
    keys = np.concatenate([np.asarray(s, dtype=np.uint64).ravel() for s in keys_by_shard] + [np.zeros(0, np.uint64)])
    states, hists = np.zeros((7, 2), dtype=np.uint64), np.zeros((6, BINS), dtype=np.uint64)
    prefix, kk = 0, int(k)
    states[0] = (0, kk)
    for r, (shift, bits) in enumerate(KTH_ROUNDS):
        top = shift + bits
        agree = keys if top >= 64 else keys[(keys >> np.uint64(top)) == np.uint64(prefix >> top)]
        digit = ((agree >> np.uint64(shift)) & np.uint64((1 << bits) - 1)).astype(np.int64)
        h = np.bincount(digit, minlength=BINS)
        hists[r] = h
        d, above = 0, 0
        for cand_d in range((1 << bits) - 1, -1, -1):
            if above + int(h[cand_d]) >= kk or cand_d == 0:
                d = cand_d
                break
            above += int(h[cand_d])
        prefix |= d << shift
        kk = (kk - above) & 0xFFFFFFFFFFFFFFFF
        states[r + 1] = (prefix, kk)
    return np.uint64(bits_of_key(prefix)), states, hists


def kth_sorted(keys_by_shard, k):
    """sorted(all keys)[-k] mapped back to a double's bits."""
    allk = sorted(int(v) for s in keys_by_shard for v in np.asarray(s, dtype=np.uint64).ravel())
    return np.uint64(bits_of_key(allk[-k]))


# -------------------------------------------------------------------------------------------------------- exact SPD case
def spd_exact_case(n, seed):
    """A = L D L^T, L unit lower bidiagonal with sub-diagonal in {0, +-1} (position-dependent, runs of at most 6 non-zeros),
    D = diag(2^e), e in [-3, 3] position-dependent.  Returns A, A^-1 (both float64, exact: asserted), d (the pivots) -- A^-1 from
    Fractions: L^-1 by its recurrence, A^-1 = L^-T D^-1 L^-1."""
    sub = [0 if i % 7 == 6 else (1 if (i * i + i // 3 + seed) % 3 else -1) for i in range(n - 1)]
    d = [Fraction(2) ** (((5 * i + seed) % 7) - 3) for i in range(n)]
    A = [[Fraction(0)] * n for _ in range(n)]
    for i in range(n):
        A[i][i] = d[i] + (sub[i - 1] ** 2 * d[i - 1] if i else 0)
        if i:
            A[i][i - 1] = A[i - 1][i] = sub[i - 1] * d[i - 1]
    # M = L^-1: M[i][i] = 1, M[i][j] = -sub[i-1] M[i-1][j]  (row i of L M = I); zero once a sub-diagonal entry is zero
    M = [dict() for _ in range(n)]
    for i in range(n):
        M[i][i] = Fraction(1)
        if i and sub[i - 1]:
            for j, v in M[i - 1].items():
                M[i][j] = -sub[i - 1] * v
    X = [[Fraction(0)] * n for _ in range(n)]
    for k in range(n):
        for i, a in M[k].items():
            for j, b in M[k].items():
                X[i][j] += a * b / d[k]
    return dict(A=_to_f64(A), X=_to_f64(X), d=np.asarray([float(v) for v in d]), A_frac=A, X_frac=X, d_frac=d, sub=sub)


def is_f64(q):
    return Fraction(float(q)) == q


def _to_f64(M):
    assert all(is_f64(v) for row in M for v in row)
    return np.asarray([[float(v) for v in row] for row in M], dtype=np.float64)


def sweep_fraction(A):
    """The symmetric sweep of spd_inverse.hip's header in Fractions: sweeping k maps A -> B, B_kk = -1/A_kk, B_ik = A_ik/A_kk,
    B_ij = A_ij - A_ik A_kj / A_kk; after all k, B = -A^-1.  Returns (-B, pivots, ok): ok is False if a pivot, an intermediate or a
    product A_ik A_kj / A_kk is not exactly a float64.  (A_ik = 0 leaves row i as it is: only the non-zero rows are visited.)"""
    n = len(A)
    B = [list(r) for r in A]
    piv, ok = [], True
    for k in range(n):
        p = B[k][k]
        piv.append(p)
        col = [B[i][k] for i in range(n)]
        nz = [i for i in range(n) if i != k and col[i] != 0]
        for i in nz:
            for j in nz:
                prod = col[i] * col[j] / p
                B[i][j] = B[i][j] - prod
                ok = ok and is_f64(prod) and is_f64(B[i][j])
        for i in nz:
            B[i][k] = B[k][i] = col[i] / p
            ok = ok and is_f64(B[i][k])
        B[k][k] = -1 / p
        ok = ok and is_f64(p) and is_f64(B[k][k]) and is_f64(col[k] / p)
    return [[-v for v in r] for r in B], piv, ok
