"""Pins tests/select_kernels_reference.py -- the plain statements tests/test_select_kernels_gpu.py holds infer_kernels.hip,
kth_select.hip and spd_inverse.hip against -- without a GPU:
  topk / topk_signed   on the committed inference goldens of BSC, DSC and TSC (the reference project's own outputs), from the
                       oracle's log-joints: the states to equality, p and the marginals to the rounding of exp.  A row whose
                       topK + 1 best contain an exact tie has no order that is a function of (value, column) upstream (NumPy's
                       introsort): its states are compared as sets within each group of equal value that the topK cut does not
                       split, and the rows where the cut splits such a group -- the only ones compared on p and m alone -- are at
                       most 5 % of each golden (BSC and DSC: no tied row at all; TSC: 4 of 50 rows tie, through repeated candidates).
  kth                  against np.sort and Python's sorted, the sign of zero through the key.
  spd_exact_case       the symmetric sweep in Fractions: every pivot, intermediate and product is a float64.
  exact-class rows     K exp(-GAP) < 2^-54 up to K = 4000.
"""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import select_kernels_reference as R
from oracle import bsc_oracle, dsc_oracle, tsc_oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -53
AN = bsc_oracle.Anneal(T=1.0, anneal_prior=False)


def _close_exp(log_ref, got, what):
    """got == exp(log_ref) up to the rounding of the log-joints' handful of operations and of exp: relative 16 u (1 + |log|)."""
    lr = np.asarray(log_ref, dtype=np.longdouble)
    want = np.exp(lr).astype(np.float64)
    tol = 16 * U * (1 + np.abs(np.where(np.isfinite(lr.astype(np.float64)), lr, 0)).astype(np.float64))
    assert np.array_equal(np.isnan(want), np.isnan(got)), what
    ok = ~np.isnan(want)
    assert (np.abs(got[ok] - want[ok]) <= tol[ok] * np.abs(want[ok]) + 1e-300).all(), (what, float(np.abs(got[ok] - want[ok]).max()))


def _tied_rows(F, topK):
    out = []
    for row in F:
        best = [row[k] for k in R.ranking(row)[:topK + 1]]
        out.append(any(a == b for a, b in zip(best, best[1:])))
    return np.asarray(out)


def _bsc_case():
    g = np.load(os.path.join(GOLDEN, "bsc_inference.npz"))
    D, H, Hp, gamma = int(g["D"]), int(g["H"]), int(g["Hprime"]), int(g["gamma"])
    cand = bsc_oracle.select_hprimes_loop(g["W"], g["y"], Hp)
    _, S, SM, state_abs = bsc_oracle.generate_state_matrix(Hp, gamma)
    F = bsc_oracle.e_step_loop(AN, g["W"], float(g["pi"]), float(g["sigma"]), np.zeros(D), g["y"], cand, SM, state_abs)
    masks = (SM.astype(np.int64) << np.arange(Hp)[None, :]).sum(axis=1).astype(np.uint16)
    return g, F, cand, masks, H, H, SM.astype(np.int8), np.array([1], np.int8)


def _dsc_case():
    g = np.load(os.path.join(GOLDEN, "dsc_inference.npz"))
    D, H, Hp, gamma = int(g["D"]), int(g["H"]), int(g["Hprime"]), int(g["gamma"])
    m = dsc_oracle.make_model(D, H, Hp, gamma, g["states"])
    cand = dsc_oracle.select_hprimes_loop(m, g["W"], g["pi"], float(g["sigma"]), g["y"])
    F = dsc_oracle.e_step_loop(AN, m, g["W"], g["pi"], float(g["sigma"]), g["y"], cand)
    masks = ((m["SM"] == 1).astype(np.int64) << np.arange(Hp)[None, :]).sum(axis=1).astype(np.uint16)
    nz = np.asarray([v for v in g["states"] if v != 0], dtype=np.int8)
    return g, F, cand, masks, H, (m["K"] - 1) * H, m["SM"].astype(np.int8), nz


@pytest.mark.parametrize("case", [_bsc_case, _dsc_case], ids=["bsc", "dsc"])
def test_topk_on_the_inference_goldens(case):
    """`topk` on the oracle's log-joints reproduces the reference project's inference(topK=5, adaptive=False): the states assembled
    from top_idx as the callers do, p = exp(top_rel) (upstream reports exp(logpj - max) without logprob), m = exp(marg)."""
    g, F, cand, masks, H, single, SM, nz = case()
    want_s = g["plain_s"]
    N, topK = want_s.shape[:2]
    ref = R.topk(F, cand, masks, H, single, topK)
    tied = _tied_rows(F, topK)
    assert tied.sum() <= 0.05 * N, tied.sum()
    s = np.zeros((N, topK, H), dtype=np.int8)
    for n in range(N):
        for r, k in enumerate(ref["top_idx"][n]):
            if 1 <= k <= single:
                s[n, r, (k - 1) % H] = nz[(k - 1) // H]
            elif k > single:
                s[n, r, cand[n]] = SM[k - single - 1]
    assert np.array_equal(s[~tied], want_s[~tied])
    _close_exp(ref["top_rel"], g["plain_p"], "p")
    _close_exp(ref["marg"], g["plain_m"], "m")


def test_topk_signed_on_the_inference_golden():
    """`topk_signed` on the TSC oracle's log-joints reproduces TSC_ET.inference(topK=5, adaptive=False) of the reference project:
    p = top_post, m and am, and the states -- to equality on the rows without a tie among their topK + 1 best, as sets within every
    group of equal probability that the topK cut does not split on the tied ones."""
    g = np.load(os.path.join(GOLDEN, "tsc_inference.npz"))
    D, H, Hp, gamma = int(g["D"]), int(g["H"]), int(g["Hprime"]), int(g["gamma"])
    m = tsc_oracle.make_model(D, H, Hp, gamma)
    cand = tsc_oracle.select_hprimes_loop(m, g["W"], float(g["pi"]), float(g["sigma"]), g["y"])
    F = tsc_oracle.e_step_loop(AN, m, g["W"], float(g["pi"]), float(g["sigma"]), g["y"], cand)
    want_s = g["plain_s"]
    N, topK = want_s.shape[:2]
    ref = R.topk_signed(F, cand, m["SM"].astype(np.int8), H, topK, 1)
    tied = ref["tie"] == 1
    assert np.array_equal(tied, _tied_rows(F, topK)), "this golden has no tie of the normalised values only"
    assert np.array_equal(ref["s"][~tied], want_s[~tied])
    p_only = 0
    for n in np.flatnonzero(tied):
        order = R.ranking(F[n])
        vals = F[n][order[:topK + 1]]
        for v in np.unique(vals[:topK]):
            sel = vals[:topK] == v
            if len(vals) > topK and vals[topK] == v:          # the cut splits this group: nothing can be said about its members
                p_only += 1
                continue
            assert sorted(map(tuple, ref["s"][n][sel])) == sorted(map(tuple, want_s[n][sel])), n
    assert p_only <= 0.05 * N, (p_only, N)
    _close_exp(ref["top_lpc"], g["plain_p"], "p")
    for k in ("m", "am"):
        got, want = ref[k].astype(np.float64), g["plain_" + k]
        w = ref["m_written"]
        assert (want[~w] == 0).all()
        # (p_s = exp(F_s - lse): the argument's rounding, u (|F| + |lse|), is the relative error of every term)
        tol = (16 * U * (1 + 2 * np.abs(F).max(axis=1))[:, None] * ref["am_mag"].astype(np.float64))[w]
        assert (np.abs(got[w] - want[w]) <= tol + 1e-300).all(), k


def test_topk_reference_on_small_rows():
    """The order (value, column) descending, NaN skipped, -1 beyond the comparable entries, last position wins."""
    F = np.array([[1.0, 3.0, 3.0, -np.inf, np.nan, -np.inf]])
    r = R.topk(F, np.array([[0, 1]]), np.array([1, 2, 3], np.uint16), 2, 2, 6)
    assert r["top_idx"].tolist() == [[2, 1, 0, 5, 3, -1]]
    assert np.isnan(r["top_lpc"][0, :5].astype(np.float64)).all() and r["top_lpc"][0, 5] == -np.inf
    assert r["top_rel"][0].tolist() == [0.0, 0.0, -2.0, -np.inf, -np.inf, -np.inf]
    F = np.array([[0.0, 5.0, 5.0, 1.0]])
    vals = np.array([[1, 0], [-1, 1], [0, -1], [1, 1]], np.int8)
    r = R.topk_signed(F, np.array([[3, 3]]), vals, 4, 2, 1)
    assert r["top_idx"].tolist() == [[2, 1]] and r["tie"].tolist() == [1]
    assert r["s"][0].tolist() == [[0, 0, 0, -1], [0, 0, 0, 1]] and r["m_written"][0].tolist() == [False, False, False, True]
    p = np.exp(F[0] - np.log(np.exp(F[0]).sum()))
    assert abs(float(r["m"][0, 3]) - (p[1] - p[2] + p[3])) < 1e-15 and abs(float(r["am"][0, 3]) - (p[1] + p[2] + p[3])) < 1e-15
    r0 = R.topk_signed(F, np.array([[3, 3]]), vals, 4, 2, 0, np.array([[4, -1]]))
    assert not r0["s_written"].any() and r0["top_post"][0].tolist() == [0, 0] and (r0["top_lpc"][0] == -np.inf).all()
    # a tie of the normalised values only
    F = np.array([[50.0, 1.0, 1.0 + 2.0 ** -52, -20.0]])
    assert R.topk_signed(F, np.array([[0]]), vals[:, :1], 1, 2, 1)["tie"].tolist() == [1]
    assert R.topk_signed(F, np.array([[0]]), vals[:, :1], 1, 1, 1)["tie"].tolist() == [0]


def test_exact_class_gap():
    """K exp(-GAP) < 2^-54 up to K = 4000: with one dominant entry and every other one -inf or at least GAP below it, the sum of
    exponentials rounds to 1 in any order and the log-sum-exp is the maximum, bit for bit."""
    assert 4000 * math.exp(-R.GAP) < 2.0 ** -54
    row = np.full(4000, 7.0 - R.GAP)
    row[1234] = 7.0
    l, m = R.lse(row)
    assert np.float64(l) == 7.0 and m == 7.0 and np.float64(np.exp(np.float64(l) - 7.0)) == 1.0


@pytest.mark.parametrize("n", [1, 5, 1000, 5003])
def test_kth_against_sort(n):
    """`kth` against np.sort on finite data (duplicates, +-0, denormals), the sign of zero through the key (np.sort orders +-0
    arbitrarily), split into two shards and with an empty one; every round's state is the prefix of the answer's key."""
    rng = np.random.RandomState(n)
    x = np.concatenate([rng.normal(size=n) * 50, [0.0, -0.0, 1e-310, -1e-310, 3.5, 3.5, -7.25]])
    rng.shuffle(x)
    keys = R.keys_of(x)
    assert [int(k) for k in keys[:50]] == [R.key_of_int(b) for b in x[:50].view(np.uint64)]
    assert np.array_equal(R.doubles_of_keys(keys).view(np.uint64), x.view(np.uint64))
    assert all(R.bits_of_key(R.key_of_int(b)) == int(b) for b in x[:50].view(np.uint64))
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(x[order], np.sort(x)) and (np.diff(keys[order].astype(np.float64)) >= 0).all()
    for k in sorted({1, 2, len(x) // 2, len(x) - 1, len(x)}):
        bits, states, hists = R.kth([keys[:len(x) // 3], keys[len(x) // 3:]], k)
        bits2, states2, hists2 = R.kth([keys[:0], keys], k)
        assert bits == bits2 and np.array_equal(states, states2) and np.array_equal(hists, hists2)
        got, want = np.array([bits]).view(np.float64)[0], np.sort(x)[-k]
        assert got == want and bits == R.kth_sorted([keys], k), (k, got, want)
        assert int(np.sort(keys)[-k]) == R.key_of_int(bits)
        key = R.key_of_int(bits)
        for r, (shift, nbits) in enumerate(R.KTH_ROUNDS):
            assert int(states[r + 1][0]) == (key >> shift) << shift and int(hists[r].sum()) >= int(states[r][1]) >= int(states[r + 1][1]) >= 1
        assert int(states[6][1]) <= int(hists[5].max()) and int(states[0][1]) == k
    zeros = R.keys_of(np.array([0.0, -0.0]))
    assert R.kth([zeros], 1)[0] == np.array([0.0]).view(np.uint64)[0] and R.kth([zeros], 2)[0] == np.array([-0.0]).view(np.uint64)[0]
    nans = np.array([0x7FF8000000000001, 0xFFF8000000000001, 0x7FF0000000000000, 0xFFF0000000000000], dtype=np.uint64)
    assert [int(R.kth([R.keys_of(nans.view(np.float64))], k)[0]) for k in (1, 2, 3, 4)] == [int(nans[i]) for i in (0, 2, 3, 1)]


@pytest.mark.parametrize("n", [33, 65, 255])
def test_spd_exact_case(n):
    """For every n used on the GPU: the symmetric sweep of spd_inverse.hip's header comment in Fractions.  Every pivot, every
    intermediate and every product A_ik A_kj / A_kk is exactly a float64 -- so any evaluation order, fused or not, gives the same
    bits --, the pivots are exactly the entries of D, and -B is A^-1 (A X = I in Fractions)."""
    c = R.spd_exact_case(n, n)
    sub, d = c["sub"], c["d_frac"]
    run = longest = 0
    for v in sub:
        run = run + 1 if v else 0
        longest = max(longest, run)
    assert longest <= 6 and set(sub) == {-1, 0, 1} and all(Fraction(1, 8) <= v <= 8 for v in d) and len(set(d)) == 7
    X, piv, ok = R.sweep_fraction(c["A_frac"])
    assert ok, "an intermediate of the sweep is not a float64"
    assert piv == d and X == c["X_frac"]
    A, Xf = c["A_frac"], c["X_frac"]
    for i in range(n):
        for j in range(n):
            assert sum(A[i][k] * Xf[k][j] for k in range(max(i - 1, 0), min(i + 2, n))) == (1 if i == j else 0)
    assert np.array_equal(c["A"], c["A"].T) and np.array_equal(c["X"], c["X"].T)
    # the refinement's first product is exact as well: every partial sum of (A X)_ij is a multiple of 2^-6 far below 2^53
    assert np.array_equal(c["A"] @ c["X"], np.eye(n))
    dadd = 0.125 * (1 + np.arange(n) % 3)
    assert np.array_equal((c["A"] - np.diag(dadd)) + np.diag(dadd), c["A"])
