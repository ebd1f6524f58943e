"""The mixture kernels (mixture_kernels.hip) through the C ABI -- pm_mix_scores_f64, pm_mix_loglik_f64, pm_mix_posterior_f64,
pm_mix_chol_f64, pm_mix_maha_f64, pm_mix_mstats_f64 (with pm_mix_stats_chunks / pm_mix_stats_len / pm_mix_mstats_work_len) -- on
padded, guarded operands at every tile edge, stride and chunk regime, against the plain longdouble reference
tests/mixture_kernels_reference.py (pinned on the CPU by tests/test_mixture_kernels_cpu.py), from both libraries.

Harness: ``Emb`` of tests/test_eval_kernels_gpu.py.  Every operand sits in a buffer with 16 guard rows before and after, a padded
leading dimension wherever the ABI has one (ldy, ldb -- shared by Bq and Bl --, lds, ldp), filled with the quiet-NaN payload
pattern.  logpj, post, rows, L_work, Linv, logdet, status, work and stats have no leading dimension: the guards before and after
are the check (`work` is exactly pm_mix_mstats_work_len long).  After every call: every guard and padding element of every output
still holds the pattern, every input is bit-unchanged, the results match the reference.  Every entry is called twice from each
library; the four results must be bit-equal (no atomics: the header's claim is a contract here).

Exact (equality with the reference, value for value; non-finite values by kind): every exact=True case's logpj, the maha result,
every entry of stats -- integers, powers of two and dyadic fractions whose every partial sum in any order is a float64, so a
difference is a wrong index, a dropped or doubled row or a leaked padding value, never rounding.  status of chol, and the NaN /
+inf / -inf pattern of every output of every case.

Bounded, against the longdouble reference (u = 2^-53, RTOL = 1e-11 of tests/test_eval_kernels_gpu.py, FLOOR = 1e-290); first-order
bounds of the kernels' own operation counts, not fitted:
  S = sum of K products (K = D for MoP, 2 D for MoG diagonal, N for the statistics): each term is rounded at most twice before it
             is added (the row scale, the square) and the chain of additions is at most K long (MFMA accumulation, then for the
             statistics the G partials in order: chunk + G <= N + 2), so |err| <= (K + 2) u sum|terms| + FLOOR, sum|terms| from the
             reference per output element.
  logpj      (S + c) coef + lp: the bound of S times |coef|, plus u (|S + c| |coef| + |lp|).  pm_mix_posterior_f64 takes S as an
             input and rounds three times: 3 u (|S + c| |coef| + |lp|).
  posteriors relative RTOL + 2 B_n, B_n the largest logpj bound among the row's finite log-joints: an error d in an argument of exp
             is a relative error d in the value, and the numerator and the row sum both move.  (-inf gives `tiny` and +inf gives
             DBL_MAX / H whatever the rounding; a value within B_n of the `tiny` clamp may be clamped on one side and not on the
             other, and both results are still equal within the bound.  No case puts a value near the overflow clamp.)
  loglik     log-sum-exp is 1-Lipschitz in the largest error of its arguments: B_n + RTOL (|lse| + sum_d |lgamma|) (libm's exp, log,
             lgamma; the online rescaling rounds a handful of times on a sum in [1, H]).
  maha       z_j = sum_k B_jk u_k with e_j = (D + 2) u sum_k |B_jk| |u_k| (u_k = y - w rounds once); mode 0: sum_j z_j^2 is off by
             at most sum_j (2 |z_j| e_j + e_j^2) + (D + 2) u sum_j z_j^2; mode 1: sum_j e_j |u_j| + (D + 2) u sum_j |z_j u_j|.
             (u . (B u) = u . (B^T u) for every B, so no value can tell B = Sinv^T from B = Sinv; the non-symmetric slot tells
             z . u from z . z and a z_j paired with the wrong u_j.)
  chol       backward error of the factorisation (Higham, Accuracy and Stability, Thm 10.3): |L L^T - A| <= (D + 2) u |L| |L|^T on
             the lower triangle; forward substitution per column gives |L X - I| <= (D + 2) u |L| |X|, hence
             |X L - I| = |X (L X - I) L ... | <= (D + 2) u (|X| |L|)^2 first order -- this is where the conditioning enters, and the
             cases are I + 0.3 B B^T / D with cond_2 <= 4 (asserted on the CPU); log det moves by tr(A^-1 dA):
             (D + 2) u (sum_ij |A^-1|_ij (|L| |L|^T)_ij + sum_j |log d_j|).  |L|, |X| from the reference.
No case is excluded from any comparison.

Worst observed error as a fraction of its bound (MI355X; 72 tests pass on the unchanged source in 6.5 s, the slowest --
test_chol[c_d300] -- in 0.9 s; the module's autouse fixture prints the table with -s).  Both libraries give the same bits in
every call, so the two columns are equal:
                              default    deterministic
  scores     logpj            0.77       0.77         (D = 1: one product and three roundings against 3 u |S| + u (...))
  scores     posteriors       0.0047     0.0047
  loglik     rows, pmf = 0    0.00084    0.00084
  loglik     rows, pmf = 1    0.000061   0.000061
  posterior  logpj            0.56       0.56
  posterior  posteriors       0.00022    0.00022
  maha       S, mode 0        0.40       0.40         (D = 1)
  maha       S, mode 1        0.43       0.43
  mstats     colsum           0.17       0.17
  mstats     Y^T P            0.45       0.45         (N = 1: a single product)
  mstats     second moments   0.46       0.46
  chol       L L^T - A        0.52       0.52         (D = 1: sqrt and one square)
  chol       Linv L - I       0.12       0.12
  chol       logdet           0.062      0.062
Nothing exceeds its bound and no test of this module fails on the unchanged source: no kernel bug was found.  The bounds that are
nearly met are the ones of single operations, where "first order" has no slack to give; the RTOL-based ones (libm) are three to
four orders of magnitude wide.

Mutants of mixture_kernels.hip, one line each, values and predicates only (a leading dimension replaced by the width reads inside
the same padded buffer; the one extra row of mutant 6 is a guard row), each built into a library of its own outside the tree and
run once against this module on the MI355X, its pm_mix_* entries in place of the default library's:
   1 `ldy` -> `D` in the `ya` pointer of the scores kernel        30 fail: test_scores and test_loglik at every shape but N = 1,
                                                                  test_row_isolation[scores]
   2 `ldp` -> `H` (sa_ld) in the Gram launch                      8: test_mstats, every kind-2 case but N = 1
   3 loader predicate `k < D` -> `k <= D - 1 - (D % 2)` (scores)   13: test_scores / test_loglik at every odd D (1, 15, 17, 33, 3)
   4 the `h < H` mask of the LL tile dropped                      6: test_loglik at H = 1, 63, 65, 130 (two shapes), 1100
   5 `exp(run_m[i] - m)` -> `exp(bm - m)` in the online lse       5: test_loglik at every H > 64
   6 `n < nend` -> `n <= nend` in the M-step loader               11: test_mstats wherever the last chunk is no multiple of 16 rows
                                                                  (t_n16 and t_g64 are: the loop never reaches row nend there)
   7 `cs` without `blockIdx.x == 0`                               0: EQUIVALENT -- every row of tiles loads the same P columns, forms
                                                                  the same sums in the same order and stores the same bits to the
                                                                  same place
   8 `sq ? z * z : z * u` swapped                                 10: test_maha, every case
   9 `g < G` -> `g < G - 1` in the reduction                      2: test_mstats[t_g2, t_g2_full] (the last chunk of t_g64 is empty)
  10 `!(d > 0.0)` -> `d < 0.0` in the Cholesky                    6: test_chol, every D.  It first SURVIVED: a NaN pivot is caught by
                                                                  isfinite, and no case had a pivot of exactly 0.  With the "zero"
                                                                  failure at a MIDDLE pivot it survived again at D > 2 (the rows
                                                                  below become NaN and the next pivot fails: the same outputs), so
                                                                  the zero sits at the last pivot now
  11 `ldy` -> `D` in the `ya` pointer of the maha kernel          10: test_maha, every case but N = 1, test_row_isolation[maha]
  12 `Y[n * ldy + col]` -> `Y[n * D + col]` (maha, mode 1)        10: the same tests
  13 `S[n * lds + h]` -> `S[n * H + h]` in the posterior kernel   7: test_posterior, every case with N > 1, test_row_isolation[posterior]
  14 `B[n * ldb + jj]` -> `B[n * NB + jj]` in the M-step loader   12: test_mstats, every case but N = 1
  15 `inf -> mx` -> `inf -> DBL_MAX` in the epilogue              6: test_scores[s_special], test_posterior at every N >= 3
  16 lgamma added in every H block (`h0 == 0` dropped)            5: test_loglik at every H > 64
  17 `double t = csr[0][tid]` -> `0.0` (column-sum phase 0)       13: test_mstats, every case
One mutant (7) is equivalent; none survives unexplained.
"""
import ctypes
import functools

import numpy as np
import pytest

import mixture_kernels_reference as R
from test_eval_kernels_gpu import GUARD_ROWS, LAYOUTS, RTOL, SENT_F64, Emb, _ld, _stream, dev  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PM_OK = 0
LD = np.longdouble
U = 2.0 ** -53
FLOOR = 1e-290
LIBS = (False, True)
WORST = {}                          # (entry, quantity, library) -> (error / bound, error, bound)
SCORE_NAMES = [n for n in R.CASES if R.CASES[n][0] == "scores"]
LOGLIK_NAMES = [n for n in R.CASES if R.CASES[n][0] in ("scores", "loglik")]
ALL_LAYOUT_CASES = ("s_mid", "m_mid", "t_n17")
PATTERN = np.array([SENT_F64], dtype=np.uint64).view(np.float64)[0]


def _lib_of(det):
    from prosper_amd import _lib
    return _lib.load(det)


def _f(x):
    with np.errstate(all="ignore"):
        return np.asarray(x, dtype=LD).astype(np.float64)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _note(entry, what, det, err, bound):
    key = (entry, what, "det" if det else "default")
    ratio = float(err) / float(bound) if bound > 0 else 0.0
    if ratio > WORST.get(key, (-1.0, 0.0, 0.0))[0]:
        WORST[key] = (ratio, float(err), float(bound))


def _pattern_equal(got, want, tag):
    got, want = np.asarray(got), _f(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (tag, "NaN pattern", np.argwhere(np.isnan(got) != np.isnan(want))[:5])
    assert np.array_equal(np.isposinf(got), np.isposinf(want)), (tag, "+inf pattern")
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), (tag, "-inf pattern")
    return np.isfinite(want)


def _exact(got, want, tag):
    """Equality with the reference, value for value, where it is finite; the same kind of non-finite value elsewhere."""
    fin = _pattern_equal(got, want, tag)
    w = _f(want)
    assert np.array_equal(np.asarray(got)[fin], w[fin]), (tag, "not equal to the reference at", np.argwhere(fin & (np.asarray(got) != w))[:8])


def _bounded(got, want, bound, entry, what, det, tag):
    """|got - want| <= bound wherever the reference is finite (the same kind of non-finite value elsewhere)."""
    fin = _pattern_equal(got, want, tag)
    if not fin.any():
        return
    g, w = np.asarray(got).astype(LD)[fin], np.asarray(want, dtype=LD)[fin]
    b = np.broadcast_to(np.asarray(bound, dtype=LD), np.shape(got))[fin]
    assert np.isfinite(_f(b)).all() and (b > 0).all(), (tag, what, "a bound is not a positive finite number")
    err = np.abs(g - w)
    i = int(np.argmax(err / b))
    _note(entry, what, det, err[i], b[i])
    assert (err <= b).all(), (tag, what, "error", float(err[i]), "bound", float(b[i]), "at", np.argwhere(fin)[i])


def _sync_rc(rc, tag):
    torch.cuda.synchronize()
    assert rc == PM_OK, (tag, rc)


def _all_equal(results, tag):
    """Two calls from each library: the same bits."""
    keys = list(results)
    first = results[keys[0]]
    for k in keys[1:]:
        for name in first:
            assert _same_bits(first[name], results[k][name]), (tag, name, "differs between", keys[0], "and", k)


def _vec(x, dev, fill=True):
    return Emb(np.asarray(x), len(x), dev, fill=fill)


# ----------------------------------------------------------------------------------------- pm_mix_scores_f64 / loglik
@functools.lru_cache(maxsize=None)
def _scores_case(name, exact, form, pmf=0, yoff=0.0):
    """Operands, reference and bounds of a scores / loglik case, computed once and shared."""
    c = R.make_case(name, exact, form=form, pmf=pmf)
    logpj, S, mag = R.scores(c["Y"], c["rs"], c["Bq"], c["Bl"], c["c"], c["coef"], c["lp"])
    K = c["D"] * (2 if c["Bq"] is not None else 1)
    fin = np.isfinite(_f(logpj))
    with np.errstate(all="ignore"):
        B = (K + 2) * U * mag * abs(c["coef"]) + U * (np.abs(S + c["c"][None, :]) * abs(c["coef"]) + np.abs(c["lp"])[None, :]) + FLOOR
    Bn = np.where(fin, B, 0).max(axis=1)                      # the largest bound among the row's finite log-joints
    post = R.posterior(logpj)
    rows, lse, lgmag = R.loglik_rows(logpj, c["Y"], c["rs"], pmf, yoff)
    with np.errstate(all="ignore"):
        Brows = Bn + RTOL * (np.abs(np.where(np.isfinite(_f(lse)), lse, 0)) + np.where(np.isfinite(_f(lgmag)), lgmag, 0)) + FLOOR
    return c, dict(logpj=logpj, B=np.where(fin, B, 1.0), post=post, Bpost=(RTOL + 2 * Bn)[:, None] * post + FLOOR, rows=rows, Brows=Brows)


def _launch_scores(dev, det, c, layout, ll=None, Y=None):
    """One call of pm_mix_scores_f64 (ll None) or pm_mix_loglik_f64 (ll = (pmf, yoff)) on guarded operands."""
    N, D, H = c["N"], c["D"], c["H"]
    ops = dict(Y=Emb(c["Y"] if Y is None else Y, _ld(D, layout, 0), dev), c=_vec(c["c"], dev), lp=_vec(c["lp"], dev))
    ldb = _ld(D, layout, 1)
    ops["Bl"] = Emb(c["Bl"], ldb, dev)
    if c["Bq"] is not None:
        ops["Bq"] = Emb(c["Bq"], ldb, dev)
    if c["rs"] is not None:
        ops["rs"] = _vec(c["rs"], dev)
    p = lambda k: ops[k].ptr if k in ops else None
    lib = _lib_of(det)
    tag = (c["form"], N, D, H, c["exact"], det, layout, ll)
    if ll is None:
        outs = dict(logpj=Emb(np.zeros((N, H)), H, dev, fill=False), post=Emb(np.zeros((N, H)), H, dev, fill=False))
        rc = lib.pm_mix_scores_f64(p("Y"), ops["Y"].ld, p("rs"), p("Bq"), p("Bl"), ldb, p("c"), c["coef"], p("lp"), N, D, H,
                                   outs["logpj"].ptr, outs["post"].ptr, _stream())
    else:
        outs = dict(rows=_vec(np.zeros(N), dev, fill=False))
        rc = lib.pm_mix_loglik_f64(p("Y"), ops["Y"].ld, p("rs"), p("Bq"), p("Bl"), ldb, p("c"), c["coef"], p("lp"), N, D, H, int(ll[0]),
                                   float(ll[1]), outs["rows"].ptr, _stream())
    _sync_rc(rc, tag)
    for k, e in outs.items():
        assert e.outside_untouched(), (tag, k, "a guard element was written")
        assert e.written(), (tag, k, "an element of the result was not written")
    for k, e in ops.items():
        assert e.unchanged(), (tag, k, "an input was written")
    return {k: e.host() for k, e in outs.items()}


def _layouts(name):
    return LAYOUTS if name in ALL_LAYOUT_CASES else ("odd",)


@pytest.mark.parametrize("name", SCORE_NAMES)
def test_scores(dev, name):
    """Both Bq forms, MoP with and without the row scale; exact inputs to equality, generic ones to the bounds; the posteriors to
    their bound in both.  `s_special`: a NaN row, a +inf, a row of -inf, -inf in all of the first H block."""
    for form in R.FORMS:
        for exact in (True, False):
            c, ref = _scores_case(name, exact, form, 0, 0.0)
            for layout in _layouts(name):
                res = {}
                for det in LIBS:
                    for rep in range(2):
                        out = res[(det, rep)] = _launch_scores(dev, det, c, layout)
                        tag = (name, form, exact, det, layout)
                        if exact:
                            _exact(out["logpj"], ref["logpj"], tag)
                        _bounded(out["logpj"], ref["logpj"], ref["B"], "scores", "logpj", det, tag)
                        _bounded(out["post"], ref["post"], ref["Bpost"], "scores", "post", det, tag)
                _all_equal(res, (name, form, exact, layout))


@pytest.mark.parametrize("name", LOGLIK_NAMES)
def test_loglik(dev, name):
    """pm_mix_loglik_f64 at the scores shapes and at H = 1100 > PM_MAX_H (three H blocks and more: the running maximum moves), pmf
    0 / 1 with yoff 0 / 1 (the lgamma term at every D tail); the special rows give NaN, +inf, -inf and a finite value."""
    assert name != "l_h1100" or R.CASES[name][3] > R.PM_MAX_H
    for form, pmf, yoff in R.LL_FORMS:
        for exact in (True, False):
            c, ref = _scores_case(name, exact, form, pmf, yoff)
            res = {}
            for det in LIBS:
                for rep in range(2):
                    out = res[(det, rep)] = _launch_scores(dev, det, c, "odd", ll=(pmf, yoff))
                    _bounded(out["rows"][0], ref["rows"], ref["Brows"], "loglik", "rows pmf=%d" % pmf, det, (name, form, pmf, yoff, exact, det))
            _all_equal(res, (name, form, pmf, yoff, exact))
            if name == "s_special":
                got, sr = res[(False, 0)]["rows"][0], R.SPECIAL_ROWS
                assert np.isnan(got[sr["nan"]]) and got[sr["pinf"]] == np.inf and got[sr["all_ninf"]] == -np.inf
                assert np.isfinite(got[sr["block1_ninf"]])


# ------------------------------------------------------------------------------------------------ pm_mix_posterior_f64
def _launch_posterior(dev, det, c, lds, S=None):
    N, H = c["N"], c["H"]
    ops = dict(S=Emb(c["S"] if S is None else S, lds, dev), c=_vec(c["c"], dev), lp=_vec(c["lp"], dev))
    outs = dict(logpj=Emb(np.zeros((N, H)), H, dev, fill=False), post=Emb(np.zeros((N, H)), H, dev, fill=False))
    rc = _lib_of(det).pm_mix_posterior_f64(ops["S"].ptr, lds, ops["c"].ptr, c["coef"], ops["lp"].ptr, N, H, outs["logpj"].ptr,
                                           outs["post"].ptr, _stream())
    tag = ("posterior", N, H, c["exact"], det, lds)
    _sync_rc(rc, tag)
    for k, e in outs.items():
        assert e.outside_untouched() and e.written(), (tag, k)
    assert all(e.unchanged() for e in ops.values()), (tag, "an input was written")
    return {k: e.host() for k, e in outs.items()}


@pytest.mark.parametrize("name", [n for n in R.CASES if R.CASES[n][0] == "posterior"])
def test_posterior(dev, name):
    """N in {1, 3, 4, 5} (four rows per workgroup), H in {1, 64, 65, 1024}, lds > H; a row with NaN, +inf and -inf and a row whose
    every weight underflows."""
    for exact in (True, False):
        c = R.make_case(name, exact)
        N, H = c["N"], c["H"]
        logpj = R.logpj_of(c["S"], c["c"], c["coef"], c["lp"])
        fin = np.isfinite(_f(logpj))
        with np.errstate(all="ignore"):
            B = 3 * U * (np.abs(c["S"].astype(LD) + c["c"][None, :]) * abs(c["coef"]) + np.abs(c["lp"])[None, :]) + FLOOR
        Bn = np.where(fin, B, 0).max(axis=1)
        post = R.posterior(logpj)
        res = {}
        for det in LIBS:
            for rep, lds in enumerate((H + 3, H + 4)):
                out = _launch_posterior(dev, det, c, lds)
                res[(det, rep)] = out
                tag = (name, exact, det, lds)
                if exact:
                    _exact(out["logpj"], logpj, tag)
                _bounded(out["logpj"], logpj, np.where(fin, B, 1.0), "posterior", "logpj", det, tag)
                _bounded(out["post"], post, (RTOL + 2 * Bn)[:, None] * post + FLOOR, "posterior", "post", det, tag)
        _all_equal(res, name)
        if N >= 3:
            assert np.array_equal(res[(False, 0)]["post"][N - 1], np.full(H, 1.0 / H)), "a row of `tiny` is 1 / H"


# ----------------------------------------------------------------------------------------------------- pm_mix_chol_f64
def _launch_chol(dev, det, S):
    """S (H, D, D) float64 with its strict upper triangles replaced by the guard pattern."""
    H, D, _ = S.shape
    A = S.copy()
    iu = np.triu_indices(D, 1)
    A[:, iu[0], iu[1]] = PATTERN
    ops = dict(S=Emb(A.reshape(H * D, D), D, dev))
    assert D == 1 or np.isnan(A[:, iu[0], iu[1]]).all()
    outs = dict(L=Emb(np.zeros((H * D, D)), D, dev, fill=False), X=Emb(np.zeros((H * D, D)), D, dev, fill=False),
                logdet=_vec(np.zeros(H), dev, fill=False), status=_vec(np.zeros(H, dtype=np.int32), dev, fill=False))
    rc = _lib_of(det).pm_mix_chol_f64(ops["S"].ptr, D, H, outs["L"].ptr, outs["X"].ptr, outs["logdet"].ptr, outs["status"].ptr, _stream())
    tag = ("chol", D, H, det)
    _sync_rc(rc, tag)
    for k, e in outs.items():
        assert e.outside_untouched(), (tag, k, "a guard element was written")
    assert outs["logdet"].written() and outs["status"].written() and ops["S"].unchanged(), tag
    return dict(L=outs["L"].host().reshape(H, D, D), X=outs["X"].host().reshape(H, D, D), logdet=outs["logdet"].host()[0],
                status=outs["status"].host()[0])


@functools.lru_cache(maxsize=None)
def _chol_ref(name):
    S, _ = R.make_case(name, False)
    out = []
    for h in range(S.shape[0]):
        L, X, ld, status = R.chol(S[h])
        assert status == 0
        aL, aX = np.abs(_f(L)), np.abs(_f(X))
        D = S.shape[1]
        LLt = aL @ aL.T
        M = aX @ aL
        with np.errstate(all="ignore"):
            logd = np.abs(2 * np.log(np.diag(aL))).sum()
        out.append(dict(ld=ld, b_res=(D + 2) * U * LLt + FLOOR, b_inv=(D + 2) * U * (M @ M) + FLOOR,
                        b_ld=(D + 2) * U * (((aX.T @ aX) * LLt).sum() + logd) + FLOOR))
    return S, out


@pytest.mark.parametrize("name", [n for n in R.CASES if R.CASES[n][0] == "chol"])
def test_chol(dev, name):
    """D in {1, 2, 17, 64} with H = 3 and D in {257, 300} (the k += 256 and i += 256 strides) with H = 2; the strict upper triangle
    of every input holds the guard pattern (never read).  L L^T against the lower triangle of A, Linv L against I, log det; the
    strict upper triangle of Linv exactly 0.  Then one component failing at pivot 0, in the middle, at D - 1, with a NaN in its
    lower triangle, and with a last pivot that is exactly 0: status 1 and logdet NaN there, and every bit of its neighbours as in
    the run without a failure."""
    S, ref = _chol_ref(name)
    H, D, _ = S.shape
    res = {}
    for det in LIBS:
        for rep in range(2):
            res[(det, rep)] = _launch_chol(dev, det, S)
    good = res[(False, 0)]
    # (L_work is scratch: only its lower triangle is the factor)
    _all_equal({k: dict(X=v["X"], logdet=v["logdet"], status=v["status"], L=np.tril(v["L"])) for k, v in res.items()}, name)
    assert np.array_equal(good["status"], np.zeros(H, dtype=np.int32)), good["status"]
    iu = np.triu_indices(D, 1)
    for h in range(H):
        L, X = np.tril(good["L"][h]).astype(LD), good["X"][h].astype(LD)
        assert np.array_equal(_bits(good["X"][h][iu]), np.zeros(len(iu[0]), dtype=np.int64)), "the strict upper triangle of Linv is not +0.0"
        assert np.isfinite(good["X"][h]).all() and np.isfinite(np.tril(good["L"][h])).all()
        A = np.tril(S[h]).astype(LD)
        for det in LIBS:
            _bounded(np.tril(_f(np.tril(L @ L.T) - A)), np.zeros((D, D)), ref[h]["b_res"], "chol", "L L^T - A", det, (name, h))
            _bounded(_f(X @ L - np.eye(D)), np.zeros((D, D)), ref[h]["b_inv"], "chol", "Linv L - I", det, (name, h))
            _bounded(np.asarray([good["logdet"][h]]), np.asarray([ref[h]["ld"]]), ref[h]["b_ld"], "chol", "logdet", det, (name, h))
    bad_h = H // 2
    for what in R.CHOL_FAILS:
        F, pivot = R.make_case(name, False, fail=(bad_h, what))
        for det in LIBS:
            out = _launch_chol(dev, det, F)
            tag = (name, what, det)
            assert np.array_equal(out["status"], np.asarray([1 if h == bad_h else 0 for h in range(H)], dtype=np.int32)), (tag, out["status"])
            assert np.isnan(out["logdet"][bad_h]), tag
            for h in range(H):
                if h != bad_h:
                    assert _same_bits(out["X"][h], good["X"][h]) and _same_bits(np.tril(out["L"][h]), np.tril(good["L"][h])), (tag, h)
                    assert _same_bits(out["logdet"][h:h + 1], good["logdet"][h:h + 1]), (tag, h)


# ----------------------------------------------------------------------------------------------------- pm_mix_maha_f64
def _launch_maha(dev, det, c, layout, Y=None):
    N, D, H = c["N"], c["D"], c["H"]
    ops = dict(Y=Emb(c["Y"] if Y is None else Y, _ld(D, layout, 0), dev), W=Emb(c["W"], D, dev), B=Emb(c["B"].reshape(H * D, D), D, dev))
    if c["mode"] is not None:
        ops["mode"] = _vec(c["mode"], dev)
    out = Emb(np.zeros((N, H)), max(_ld(H, layout, 1), H + 1), dev, fill=False)          # lds > H in every layout
    rc = _lib_of(det).pm_mix_maha_f64(ops["Y"].ptr, ops["Y"].ld, ops["W"].ptr, ops["B"].ptr, ops["mode"].ptr if "mode" in ops else None,
                                      N, D, H, out.ptr, out.ld, _stream())
    tag = ("maha", N, D, H, c["exact"], det, layout)
    _sync_rc(rc, tag)
    assert out.outside_untouched() and out.written(), (tag, "guards / padding of S")
    assert all(e.unchanged() for e in ops.values()), (tag, "an input was written")
    return dict(S=out.host())


@pytest.mark.parametrize("name", [n for n in R.CASES if R.CASES[n][0] == "maha"])
def test_maha(dev, name):
    """N in {1, 64, 65}, D in {1, 15, 17, 64, 65, 130} (one, a ragged second and a ragged third 64-column chunk), H in {1, 3}; mode
    NULL, all 0, and mixed with a non-symmetric B in the mode-1 slot; lds > H."""
    for mode_kind in ("null", "zeros", "mixed"):
        for exact in (True, False):
            c = R.make_case(name, exact, mode_kind=mode_kind)
            D, H = c["D"], c["H"]
            S, Z, Zmag, Uu = R.maha(c["Y"], c["W"], c["B"], c["mode"])
            e = (D + 2) * U * Zmag
            b0 = (2 * np.abs(Z) * e + e * e).sum(axis=2) + (D + 2) * U * (Z * Z).sum(axis=2)
            b1 = (e * Uu).sum(axis=2) + (D + 2) * U * np.abs(Z * Uu).sum(axis=2)
            sq = np.asarray([c["mode"] is None or c["mode"][h] == 0 for h in range(H)])
            bound = np.where(sq[None, :], b0, b1) + FLOOR
            for layout in _layouts(name):
                res = {}
                for det in LIBS:
                    for rep in range(2):
                        out = res[(det, rep)] = _launch_maha(dev, det, c, layout)
                        tag = (name, mode_kind, exact, det, layout)
                        if exact:
                            _exact(out["S"], S, tag)
                        _bounded(out["S"], S, bound, "maha", "S mode 1" if mode_kind == "mixed" else "S mode 0", det, tag)
                _all_equal(res, (name, mode_kind, exact, layout))


# --------------------------------------------------------------------------------------------------- pm_mix_mstats_f64
def _launch_mstats(dev, det, c, layout):
    N, D, H, kind = c["N"], c["D"], c["H"], c["kind"]
    lib = _lib_of(det)
    ops = dict(Y=Emb(c["Y"], _ld(D, layout, 0), dev), P=Emb(c["P"], _ld(H, layout, 1), dev))
    if c["rs"] is not None:
        ops["rs"] = _vec(c["rs"], dev)
    wl, L = int(lib.pm_mix_mstats_work_len(N, D, H, kind)), int(lib.pm_mix_stats_len(D, H, kind))
    assert wl == R.work_len(N, D, H, kind) and L == R.stats_len(D, H, kind)
    work, stats = _vec(np.zeros(wl), dev, fill=False), _vec(np.zeros(L), dev, fill=False)
    rc = lib.pm_mix_mstats_f64(ops["Y"].ptr, ops["Y"].ld, ops["P"].ptr, ops["P"].ld, ops["rs"].ptr if "rs" in ops else None, N, D, H, kind,
                               work.ptr, stats.ptr, _stream())
    tag = ("mstats", N, D, H, kind, c["rs"] is not None, c["exact"], det, layout)
    _sync_rc(rc, tag)
    assert work.outside_untouched(), (tag, "a guard element of work was written")
    assert stats.outside_untouched() and stats.written(), (tag, "stats")
    assert all(e.unchanged() for e in ops.values()), (tag, "an input was written")
    return dict(stats=stats.host()[0])


@pytest.mark.parametrize("name", list(R.MSTATS_CASES))
def test_mstats(dev, name):
    """Kinds 0 (with and without the row scale), 1 and 2 in every chunk regime -- asserted here from pm_mix_stats_chunks: G, the
    chunk, the rows of the last non-empty chunk, the empty trailing chunks -- on padded ldy and ldp; exact inputs to equality in
    every entry, generic ones to (N + 2) u sum|terms|."""
    N, D, H, kinds, G, chunk, empty, last = R.MSTATS_CASES[name]
    for kind in kinds:
        k = 0 if kind == "0rs" else kind
        for det in LIBS:
            g = int(_lib_of(det).pm_mix_stats_chunks(N, D, H, k))
            rows = [max(0, min(N, (i + 1) * R.chunk_rows(N, g)) - i * R.chunk_rows(N, g)) for i in range(g)]
            assert (g, R.chunk_rows(N, g)) == (G, chunk), (name, kind, g)
            assert rows.count(0) == empty and rows[g - empty - 1] == last and all(r == 0 for r in rows[g - empty:]), (name, rows)
        for exact in (True, False):
            c = R.make_case(name, exact, kind=kind)
            st, mag = R.mstats(c["Y"], c["P"], c["rs"], c["kind"])
            bound = (N + 2) * U * mag + FLOOR
            for layout in _layouts(name):
                res = {}
                for det in LIBS:
                    for rep in range(2):
                        out = res[(det, rep)] = _launch_mstats(dev, det, c, layout)
                        tag = (name, kind, exact, det, layout)
                        if exact:
                            _exact(out["stats"], st, tag)
                        for what, sl in (("colsum", slice(0, H)), ("Y^T P", slice(H, H + D * H)), ("second moments", slice(H + D * H, None))):
                            if len(st[sl]):
                                _bounded(out["stats"][sl], st[sl], bound[sl], "mstats", what, det, tag)
                _all_equal(res, (name, kind, exact, layout))


# -------------------------------------------------------------------------------------------------------- row isolation
def _others(a):
    keep = np.ones(65, dtype=bool)
    keep[list(R.ISOLATION_ROWS)] = False
    return np.asarray(a)[keep]


@pytest.mark.parametrize("entry", ["scores", "loglik", "maha", "posterior"])
def test_row_isolation(dev, entry):
    """N = 65: a NaN row, a +inf row and a 1e300 row at tile positions 0, 31 and 64 (the last one alone in the second tile, where
    the clamped loader rows repeat it).  Every other row equals the same call without them, bit for bit."""
    for det in LIBS:
        if entry in ("scores", "loglik"):
            for form, pmf, yoff in R.LL_FORMS[:4]:
                c = R.make_case("s_n65", False, form=form, pmf=pmf)
                ll = (pmf, yoff) if entry == "loglik" else None
                clean = _launch_scores(dev, det, c, "odd", ll=ll)
                dirty = _launch_scores(dev, det, c, "odd", ll=ll, Y=R.isolation_rows(c["Y"]))
                for k in clean:
                    a, b = (clean[k][0], dirty[k][0]) if k == "rows" else (clean[k], dirty[k])
                    assert _same_bits(_others(a), _others(b)), (entry, form, k, det)
                    assert not np.isfinite(np.asarray(b)[R.ISOLATION_ROWS[0]]).any() or k == "post", (entry, form, k)
        elif entry == "maha":
            c = R.make_case("m_n65", False, mode_kind="mixed")
            clean = _launch_maha(dev, det, c, "odd")
            dirty = _launch_maha(dev, det, c, "odd", Y=R.isolation_rows(c["Y"]))
            assert _same_bits(_others(clean["S"]), _others(dirty["S"])), (entry, det)
            assert np.isnan(dirty["S"][R.ISOLATION_ROWS[0]]).all()
        else:
            c = R.posterior_case(65, 65, False)
            clean = _launch_posterior(dev, det, c, 68)
            dirty = _launch_posterior(dev, det, c, 68, S=R.isolation_rows(c["S"]))
            for k in clean:
                assert _same_bits(_others(clean[k]), _others(dirty[k])), (entry, k, det)


@pytest.fixture(scope="module", autouse=True)
def _report_worst_errors():
    """After the module's tests: the largest error / bound of every bounded comparison that ran, per entry, quantity and library
    (-s shows it).  Not a check of its own: each comparison asserted its bound where it was made."""
    yield
    for key in sorted(WORST):
        ratio, err, bound = WORST[key]
        print("worst %-10s %-16s %-7s err %.3e  bound %.3e  ratio %.2e" % (key + (err, bound, ratio)))
