"""tests/mixture_kernels_reference.py pinned without a device, and what tests/test_mixture_kernels_gpu.py relies on:

* the reference against the committed outputs of the original code (tests/golden/mixture_step_*.npz: logpj, posteriors_h, and the
  M-step's parameters rebuilt from `mstats` by the formulas of MoG.M_step / MoP.M_step) and against the float64 restatements of
  tests/test_mixture_gpu.py (np_logpj_diag, np_logpj_full, np_logpj_mop, np_posterior);
* the host-only entries pm_mix_stats_len, pm_mix_stats_chunks and pm_mix_mstats_work_len equal to the reference's restatement
  over a sweep, and every M-step case in the regime it is meant for (G, chunk, ragged last K step, empty trailing chunks);
* the exact=True operands exact in the reference's sense, the generic ones with mixed signs, the Cholesky cases well
  conditioned, the special rows what they are named;
* the argument checks of the launchers that nothing asserted yet.  All of them return before anything is launched (the pointers
  are host dummies).  pm_mix_loglik_f64 has NO bound on H: with valid arguments and H > PM_MAX_H it launches, so that row is not
  here -- the GPU module runs it at H = 1100."""
import ctypes

import numpy as np
import pytest

import mixture_kernels_reference as R
from conftest import golden
from test_mixture_gpu import STEP_CASES, np_logpj_diag, np_logpj_full, np_logpj_mop, np_posterior

PM_OK, PM_EINVAL, PM_ERANGE = 0, -1, -2
LD = np.longdouble
TINY = np.finfo(np.float64).tiny
EPS = np.finfo(np.float64).eps


def _lib():
    from prosper_amd import _lib
    return _lib.load()


def _f(x):
    with np.errstate(all="ignore"):
        return np.asarray(x, dtype=LD).astype(np.float64)


def _same_pattern(a, b):
    return (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b))
            and np.array_equal(np.isneginf(a), np.isneginf(b)))


# ------------------------------------------------------------------------------------------- against the golden fixtures
def _golden_logpj(g):
    """The reference's log-joints of a fixture, from the operands the host layer hands to the kernels (MoG.posterior,
    MoP._posterior); returns (logpj, error scale or None, components that took the host inverse)."""
    beta = 1.0 / float(g["T"])
    W = np.asarray(g["in_W"], dtype=np.float64)
    y = np.asarray(g["y"], dtype=np.float64)
    H = W.shape[1]
    with np.errstate(all="ignore"):
        lp = np.log(g["in_pies"]) * beta
        if "sigmas_sq_type" not in g:                                    # MoP
            A, D = float(g["A"]), W.shape[0]
            logW = np.log(W.T)
            if np.isnan(A):
                return R.scores(y, None, None, logW, -np.sum(W, 0), beta, lp)[0], None, []
            rs = (A - D) / (np.sum(y, 1) + EPS)
            c = np.sum(logW, 1)
            return R.scores(y, rs, None, np.where(np.isneginf(logW), 0.0, logW), c, beta, lp)[0], None, []
        sig = np.asarray(g["in_sigmas_sq"], dtype=np.float64)
        if str(g["sigmas_sq_type"]) == "diagonal":
            Bq = 1.0 / sig
            c = np.sum(W.T ** 2 * Bq, 1) + np.sum(np.log(sig), 1)
            c[(sig <= 0).any(1)] = np.nan
            scale = ((y ** 2) @ Bq.T + np.sum(W.T ** 2 * Bq, 1)[None, :]) * beta
            return R.scores(y, None, Bq, -2.0 * W.T * Bq, c, -beta, lp)[0], scale, []
        D = W.shape[0]
        B, mode, logdet, fb = np.zeros((H, D, D)), np.zeros(H, dtype=np.int32), np.zeros(H), []
        for h in range(H):
            L, X, ld, status = R.chol(sig[h])
            if status == 0:
                B[h], logdet[h] = _f(X), float(ld)
            else:                                                        # the host inverse, as MoG._full_factors takes it
                B[h], mode[h], logdet[h] = np.linalg.inv(sig[h]).T, 1, np.linalg.slogdet(sig[h])[1]
                fb.append(h)
        S = R.maha(y, W.T, B, mode)[0]
        return R.logpj_of(S, logdet, -beta, lp), None, fb


@pytest.mark.parametrize("case", STEP_CASES)
def test_reference_matches_the_golden_estep(case):
    g = golden("mixture_step_%s.npz" % case)
    lp, scale, fb = _golden_logpj(g)
    assert fb == ([2] if case.startswith("fallback") else [])
    ref = g["logpj"]
    got = _f(lp)
    assert _same_pattern(got, ref)
    fin = np.isfinite(ref)
    atol = 1e-13 * (scale[fin] if scale is not None else np.abs(ref[fin]).max(initial=1.0))
    rtol = np.full(ref.shape, 1e-10)
    rtol[:, fb] = 1e-8
    assert np.all(np.abs(got[fin] - ref[fin]) <= rtol[fin] * np.abs(ref[fin]) + atol), np.abs(got[fin] - ref[fin]).max()
    # the epilogue, from the fixture's own log-joints
    np.testing.assert_allclose(_f(R.posterior(ref)), g["posteriors_h"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(_f(R.posterior(ref)), np_posterior(ref.copy(), ref.shape[1]), rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("case", STEP_CASES)
def test_reference_mstats_rebuild_the_golden_mstep(case):
    """The M-step's outputs from R.mstats of (y, the fixture's posteriors) by the formulas of MoG.M_step / MoP.M_step."""
    g = golden("mixture_step_%s.npz" % case)
    y, P = np.asarray(g["y"], dtype=np.float64), np.asarray(g["posteriors_h"], dtype=np.float64)
    D, H = int(g["D"]), int(g["H"])
    to_learn = [str(x) for x in g["to_learn"]]
    out = {k[4:]: np.array(v) for k, v in g.items() if k.startswith("out_")}
    new = {k[3:]: np.array(v) for k, v in g.items() if k.startswith("in_")}          # what is not learned is handed through
    if "sigmas_sq_type" not in g:
        A = float(g["A"])
        rs = None if np.isnan(A) else (A - D) / (np.sum(y, 1) + EPS)
        st = _f(R.mstats(y, P, rs, R.KIND_MOP)[0])
        colsum = st[:H]
        if "W" in to_learn:
            W_num = st[H:].reshape(D, H)
            if np.isnan(A):
                sp = colsum
            else:
                W_num = W_num + colsum[None, :]
                sp = np.sum(W_num, 0) / A + EPS
            new["W"] = W_num / sp[None, :] + EPS
        if "pies" in to_learn:
            new["pies"] = (colsum + TINY) / np.sum(colsum + TINY)
    else:
        full = str(g["sigmas_sq_type"]) == "full"
        st = _f(R.mstats(y, P, None, R.KIND_FULL if full else R.KIND_DIAG)[0])
        sp = st[:H] + TINY
        W = np.asarray(g["in_W"], dtype=np.float64)
        if "W" in to_learn:
            W = new["W"] = st[H:H + D * H].reshape(D, H) / sp[None, :]
        if "sigmas_sq" in to_learn:
            if full:
                sig = st[H + D * H:].reshape(H, D, D) / sp[:, None, None]
                for h in range(H):
                    sig[h] -= np.outer(W[:, h], W[:, h])
            else:
                sig = st[H + D * H:].reshape(D, H).T / sp[:, None] - W.T ** 2
            new["sigmas_sq"] = sig
        if "pies" in to_learn:
            new["pies"] = sp / np.sum(sp)
    assert sorted(new) == sorted(out)
    for k in out:
        np.testing.assert_allclose(new[k], out[k], rtol=1e-9, atol=1e-12 * max(1.0, np.abs(out[k]).max()), err_msg=k)


def test_reference_matches_the_float64_restatements():
    """np_logpj_diag / np_logpj_mop / np_logpj_full of tests/test_mixture_gpu.py, at D = 17, H = 5, N = 23."""
    rng = np.random.RandomState(3)
    N, D, H, beta = 23, 17, 5, 1 / 1.3
    W = rng.uniform(1.0, 3.0, size=(D, H))
    y = W.T[rng.randint(H, size=N)] + 0.5 * rng.normal(size=(N, D))
    pies = rng.uniform(0.5, 1.5, H)
    pies /= pies.sum()
    lp = np.log(pies) * beta
    sig = rng.uniform(0.5, 1.5, (H, D))
    Bq = 1.0 / sig
    got = R.scores(y, None, Bq, -2.0 * W.T * Bq, np.sum(W.T ** 2 * Bq, 1) + np.sum(np.log(sig), 1), -beta, lp)[0]
    ref = np_logpj_diag(y, W, sig, pies, beta)
    scale = ((y ** 2) @ Bq.T + np.sum(W.T ** 2 * Bq, 1)[None, :]).max()
    assert np.abs(_f(got) - ref).max() <= 1e-13 * scale
    np.testing.assert_allclose(_f(R.posterior(got)), np_posterior(ref.copy(), H), rtol=1e-10, atol=1e-300)
    yc = np.floor(np.abs(y) * 2)
    got = R.scores(yc, None, None, np.log(W.T), -W.sum(0), beta, lp)[0]
    np.testing.assert_allclose(_f(got), np_logpj_mop(yc, W, pies, beta), rtol=1e-12)
    full = np.empty((H, D, D))
    B, logdet = np.empty((H, D, D)), np.empty(H)
    for h in range(H):
        M = rng.normal(size=(D, D)) / np.sqrt(D)
        full[h] = np.eye(D) + 0.3 * M @ M.T
        L, X, ld, status = R.chol(full[h])
        assert status == 0
        B[h], logdet[h] = _f(X), float(ld)
        np.testing.assert_allclose(_f(L), np.linalg.cholesky(full[h]), rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(logdet[h], np.linalg.slogdet(full[h])[1], rtol=1e-12, atol=1e-14)
    ref = np_logpj_full(y, W, full, pies, beta)
    got = R.logpj_of(R.maha(y, W.T, B, None)[0], logdet, -beta, lp)
    np.testing.assert_allclose(_f(got), ref, rtol=1e-11)
    # mode 1 with B = Sinv^T of a NON-symmetric "inverse": u . (u Sinv), and not u . (Sinv u)
    Sinv = rng.normal(size=(H, D, D))
    mode = np.ones(H, dtype=np.int32)
    got = R.maha(y, W.T, np.transpose(Sinv, (0, 2, 1)), mode)[0]
    for h in range(H):
        u = y - W[:, h]
        np.testing.assert_allclose(_f(got[:, h]), np.sum((u @ Sinv[h]) * u, 1), rtol=1e-11, atol=1e-11)


def test_loglik_rows_conventions():
    z = np.array([[0.0, -1.0, 2.0], [np.nan, np.inf, 0.0], [1.0, np.inf, -np.inf], [-np.inf] * 3, [-np.inf, -np.inf, 5.0]])
    rows, lse, _ = R.loglik_rows(z)
    assert np.isnan(rows[1]) and rows[2] == np.inf and rows[3] == -np.inf and float(rows[4]) == 5.0
    assert abs(float(rows[0]) - np.log(np.exp(z[0]).sum())) < 1e-15
    Y = np.array([[0.0, 3.0], [2.0, 1.0], [1.0, 1.0], [0.0, 0.0], [4.0, 0.0]])
    rs = np.array([0.5, 1.0, 2.0, 1.0, 1.0])
    rows, lse, mag = R.loglik_rows(z, Y, rs, 1, 1.0)
    import math
    want = sum(math.lgamma(v) for v in (0.5 * 0.0 + 2.0, 0.5 * 3.0 + 2.0))
    assert abs(float(lse[0] - rows[0]) - want) < 1e-15 and float(mag[0]) >= want


# ------------------------------------------------------------------------------------------------------- host-only entries
def test_host_entries_equal_the_restatement():
    lib = _lib()
    Ns = [1, 15, 16, 17, 255, 256, 511, 512, 600, 1023, 4096, 16400, 200000, 5000000]
    DH = [(1, 1), (4, 3), (5, 3), (33, 40), (63, 65), (64, 64), (65, 63), (65, 130), (128, 64), (300, 2), (1024, 256), (1024, 1024),
          (2000, 1100), (6, 30000), (3, 70000)]
    for kind in (0, 1, 2):
        for D, H in DH:
            assert lib.pm_mix_stats_len(D, H, kind) == R.stats_len(D, H, kind)
            for N in Ns:
                G = lib.pm_mix_stats_chunks(N, D, H, kind)
                assert G == R.stats_chunks(N, D, H, kind), (N, D, H, kind)
                assert lib.pm_mix_mstats_work_len(N, D, H, kind) == R.work_len(N, D, H, kind)
                assert 1 <= G <= 64 and (G == 1 or N // G >= 256)
    for bad in ((0, 4, 2, 0), (8, 0, 2, 0), (8, 4, 0, 0), (8, 4, 2, 3), (8, 4, 2, -1)):
        assert lib.pm_mix_stats_chunks(*bad) == R.stats_chunks(*bad) == -1
        assert lib.pm_mix_mstats_work_len(*bad) == R.work_len(*bad) == -1
    assert lib.pm_mix_stats_len(0, 2, 0) == R.stats_len(0, 2, 0) == -1


@pytest.mark.parametrize("name", list(R.MSTATS_CASES))
def test_mstats_cases_are_in_their_regime(name):
    """G, the chunk, the rows of the last non-empty chunk and the number of empty trailing chunks, from the library itself."""
    lib = _lib()
    N, D, H, kinds, G, chunk, empty, last = R.MSTATS_CASES[name]
    for kind in kinds:
        k = 0 if kind == "0rs" else kind
        assert lib.pm_mix_stats_chunks(N, D, H, k) == G, (name, kind)
        g, ch, rows = R.chunk_layout(N, D, H, k)
        assert (g, ch) == (G, chunk) and sum(rows) == N
        assert sum(1 for r in rows if r == 0) == empty and all(r == 0 for r in rows[G - empty:]) and all(r > 0 for r in rows[:G - empty])
        assert rows[G - empty - 1] == last
    if name in ("t_g2", "t_g2_full"):
        assert G == 2 and last % R.BK != 0 and D <= 64 and H <= 64          # a ragged last K step in the second chunk
    if name == "t_g64":
        assert G == 64 and empty == 3 and 61 * chunk > N
    if name.startswith("t_d"):
        assert G == 1 and (D % 64 in (1, 63)) and (2 in kinds or H % 64 in (1, 2, 63))
    if name == "t_g2_full":
        assert kinds == (2,) and H == 3                                   # blockIdx.z = g * H + h carries both indices


# ------------------------------------------------------------------------------------------------------ the cases' data
SCORE_NAMES = [n for n in R.CASES if R.CASES[n][0] in ("scores", "loglik")]


@pytest.mark.parametrize("name", SCORE_NAMES)
def test_scores_cases(name):
    """exact=True operands are exact (make_case asserts it; restated here from the returned operands), generic ones have
    both signs in every row of Y and Bl, |c| <= 1/4 and every sum of magnitudes at least D / 16 (no entry's bound rests on a
    vanishing scale)."""
    entry, N, D, H = R.CASES[name]
    for form, pmf, _ in R.LL_FORMS:
        if name == "s_special":
            continue
        c = R.make_case(name, True, form=form, pmf=pmf)
        logpj, S, mag = R.scores(c["Y"], c["rs"], c["Bq"], c["Bl"], c["c"], c["coef"], c["lp"])
        assert R.exact_ok((mag + np.abs(c["c"])[None, :]) * abs(c["coef"]) + np.abs(c["lp"])[None, :], c["bits"])
        assert R.is_multiple(logpj, c["bits"]) and np.array_equal(_f(logpj).astype(LD), logpj)
        assert float(np.abs(logpj).max()) < 600                          # no exp near float64's overflow: no clamp is ambiguous
        assert not pmf or (c["Y"] >= 0).all()
        g = R.make_case(name, False, form=form, pmf=pmf)
        assert (g["Y"].shape, g["Bl"].shape) == ((N, D), (H, D))
        if D >= 15 and not pmf:
            assert ((g["Y"] < 0).any(axis=1) & (g["Y"] > 0).any(axis=1)).all()
        if D >= 15:
            assert ((g["Bl"] < 0).any(axis=1) & (g["Bl"] > 0).any(axis=1)).all()
        _, _, gmag = R.scores(g["Y"], g["rs"], g["Bq"], g["Bl"], g["c"], g["coef"], g["lp"])
        assert float(np.abs(g["c"]).max()) <= 0.25 and float(gmag.min()) >= 0.0625 * D


def test_special_rows_are_what_they_are_named():
    N, H = R.CASES["s_special"][1], R.CASES["s_special"][3]
    assert R.cdiv(H, R.BT) == 3
    for exact in (True, False):
        for form, pmf, yoff in R.LL_FORMS:
            c = R.make_case("s_special", exact, form=form, pmf=pmf)
            z = _f(R.scores(c["Y"], c["rs"], c["Bq"], c["Bl"], c["c"], c["coef"], c["lp"])[0])
            sr = R.SPECIAL_ROWS
            assert np.isnan(z[sr["nan"]]).all()
            assert np.isposinf(z[sr["pinf"], 7]) and np.isfinite(np.delete(z[sr["pinf"]], 7)).all()
            assert np.isneginf(z[sr["all_ninf"]]).all()
            assert np.isneginf(z[sr["block1_ninf"], :R.BT]).all() and np.isfinite(z[sr["block1_ninf"], R.BT:]).all()
            rest = np.delete(z, list(sr.values()), axis=0)
            assert np.isfinite(rest).all()
            where = np.argmax(rest, axis=1) // R.BT
            assert (where == 1).any(), "no row has its maximum in the second of the three H blocks"
            rows = _f(R.loglik_rows(z, c["Y"], c["rs"], pmf, yoff)[0])
            assert np.isnan(rows[sr["nan"]]) and rows[sr["pinf"]] == np.inf and rows[sr["all_ninf"]] == -np.inf
            assert np.isfinite(rows[sr["block1_ninf"]]) and np.isfinite(np.delete(rows, list(sr.values()))).all()


def test_posterior_maha_mstats_cases_are_exact():
    for name, (entry, N, D, H) in R.CASES.items():
        if entry == "posterior":
            c = R.make_case(name, True)
            z = R.logpj_of(c["S"], c["c"], c["coef"], c["lp"])
            fin = np.isfinite(_f(z))
            assert R.is_multiple(np.where(fin, z, 0), c["bits"])
        if entry == "maha":
            for mk in ("null", "zeros", "mixed"):
                c = R.make_case(name, True, mode_kind=mk)
                S, Z, Zmag, Uu = R.maha(c["Y"], c["W"], c["B"], c["mode"])
                tot = (Zmag * Zmag).sum(axis=2)                           # >= every partial sum of z^2 and of |z u|
                assert R.exact_ok(tot, 0) and R.is_multiple(S, 0) and np.array_equal(_f(S).astype(LD), S)
                if mk == "mixed" and D > 1:
                    # u . (B u) = u . (B^T u) for EVERY B: no value can tell B = Sinv^T from B = Sinv.  What the non-symmetric
                    # slot does tell apart is z . u from z . z, and z_j paired with another u_j'
                    h = H // 2
                    other = R.maha(c["Y"], c["W"], np.transpose(c["B"], (0, 2, 1)), c["mode"])[0]
                    assert np.array_equal(other[:, h], S[:, h]) and not np.array_equal(c["B"][h], c["B"][h].T)
                    sq = R.maha(c["Y"], c["W"], c["B"], None)[0]
                    assert (sq[:, h] != S[:, h]).any()
    for name, (N, D, H, kinds, *_r) in R.MSTATS_CASES.items():
        for kind in kinds:
            c = R.make_case(name, True, kind=kind)
            st, mag = R.mstats(c["Y"], c["P"], c["rs"], c["kind"])
            assert R.exact_ok(mag, c["bits"]) and R.is_multiple(st, c["bits"]) and np.array_equal(_f(st).astype(LD), st)
            g = R.make_case(name, False, kind=kind)
            assert (g["Y"] < 0).any() and (g["Y"] > 0).any() and (g["P"] > 0).all()


@pytest.mark.parametrize("name", [n for n in R.CASES if R.CASES[n][0] == "chol"])
def test_chol_cases_are_well_conditioned(name):
    """cond_2 of every covariance is a few units; the failing variants fail where they are meant to (and only there)."""
    _, _, D, H = R.CASES[name]
    S, _ = R.make_case(name, False)
    for h in range(H):
        assert R.spectral_cond(S[h]) <= 4.0, (name, h)
        L, X, ld, status = R.chol(S[h])
        assert status == 0
        res = np.abs(np.tril(L @ L.T) - np.tril(S[h].astype(LD))).max()
        assert float(res) <= 1e-17 and float(np.abs(X @ L - np.eye(D)).max()) <= 1e-16
        junk = np.triu(np.full((D, D), np.nan), 1) + np.tril(S[h])        # the upper triangle is not read
        assert np.array_equal(R.chol(junk)[0], L)
    for what in R.CHOL_FAILS:
        F, pivot = R.make_case(name, False, fail=(H // 2, what))
        if what == "zero":                                                # the pivot is exactly 0, in float64 as in longdouble
            Lz = R.chol(F[H // 2])[0]
            assert float(F[H // 2][pivot, pivot]) - float((Lz[pivot, :pivot] ** 2).sum()) == 0.0
        for h in range(H):
            status = R.chol(F[h])[3]
            assert status == (1 if h == H // 2 else 0), (name, what, h)
            assert h == H // 2 or np.array_equal(F[h], S[h])


# ------------------------------------------------------------------------------------------------------- argument checks
def _dummy(n=64):
    buf = (ctypes.c_double * n)()
    return buf, ctypes.c_void_p(ctypes.addressof(buf))


def test_argument_checks_return_before_any_launch():
    lib = _lib()
    keep, p = _dummy()
    N, D, H = 4, 3, 2
    big = R.PM_MAX_H + 1
    sc = dict(Y=p, ldy=D, rs=None, Bq=None, Bl=p, ldb=D, c=p, coef=1.0, lp=p, N=N, D=D, H=H, logpj=p, post=p)

    def scores(**o):
        a = dict(sc, **o)
        return lib.pm_mix_scores_f64(a["Y"], a["ldy"], a["rs"], a["Bq"], a["Bl"], a["ldb"], a["c"], a["coef"], a["lp"], a["N"], a["D"],
                                     a["H"], a["logpj"], a["post"], None)

    def loglik(pmf=0, **o):
        a = dict(sc, **o)
        return lib.pm_mix_loglik_f64(a["Y"], a["ldy"], a["rs"], a["Bq"], a["Bl"], a["ldb"], a["c"], a["coef"], a["lp"], a["N"], a["D"],
                                     a["H"], pmf, 0.0, a["post"], None)

    for fn in (scores, loglik):
        assert fn(ldy=D - 1) == PM_EINVAL and fn(ldb=D - 1) == PM_EINVAL
        assert fn(Bq=p, rs=p) == PM_EINVAL
        assert fn(N=0) == PM_EINVAL and fn(D=0) == PM_EINVAL and fn(H=0) == PM_EINVAL
    assert loglik(pmf=1, Bq=p) == PM_EINVAL
    assert loglik(post=None) == PM_EINVAL
    assert scores(H=big) == PM_ERANGE and scores(H=big, Bq=p) == PM_ERANGE
    assert scores(H=big, ldy=D - 1) == PM_EINVAL                          # the argument checks come first
    # (pm_mix_loglik_f64 with H > PM_MAX_H and valid arguments launches: tests/test_mixture_kernels_gpu.py runs H = 1100)
    post = lambda **o: (lambda a: lib.pm_mix_posterior_f64(a["S"], a["lds"], a["c"], 1.0, a["lp"], a["N"], a["H"], a["logpj"], a["post"],
                                                           None))(dict(dict(S=p, lds=H, c=p, lp=p, N=N, H=H, logpj=p, post=p), **o))
    assert post(lds=H - 1) == PM_EINVAL and post(H=big, lds=big) == PM_ERANGE and post(H=big, lds=big - 1) == PM_EINVAL
    assert post(N=0) == PM_EINVAL and post(logpj=None) == PM_EINVAL
    maha = lambda **o: (lambda a: lib.pm_mix_maha_f64(a["Y"], a["ldy"], a["W"], a["B"], a["mode"], a["N"], a["D"], a["H"], a["S"], a["lds"],
                                                      None))(dict(dict(Y=p, ldy=D, W=p, B=p, mode=None, N=N, D=D, H=H, S=p, lds=H), **o))
    assert maha(ldy=D - 1) == PM_EINVAL and maha(lds=H - 1) == PM_EINVAL
    assert maha(H=65536, lds=65536) == PM_ERANGE and maha(H=65536, lds=65535) == PM_EINVAL
    assert maha(W=None) == PM_EINVAL and maha(B=None) == PM_EINVAL and maha(S=None) == PM_EINVAL
    ms = lambda **o: (lambda a: lib.pm_mix_mstats_f64(a["Y"], a["ldy"], a["P"], a["ldp"], a["rs"], a["N"], a["D"], a["H"], a["kind"], a["work"],
                                                      a["stats"], None))(dict(dict(Y=p, ldy=D, P=p, ldp=H, rs=None, N=N, D=D, H=H, kind=0,
                                                                                   work=p, stats=p), **o))
    assert ms(ldy=D - 1) == PM_EINVAL and ms(ldp=H - 1) == PM_EINVAL
    assert ms(rs=p, kind=1) == PM_EINVAL and ms(rs=p, kind=2) == PM_EINVAL
    assert ms(kind=3) == PM_EINVAL and ms(kind=-1) == PM_EINVAL and ms(work=None) == PM_EINVAL and ms(stats=None) == PM_EINVAL
    chol = lambda **o: (lambda a: lib.pm_mix_chol_f64(a["S"], a["D"], a["H"], a["L"], a["X"], a["ld"], a["st"], None))(
        dict(dict(S=p, D=D, H=H, L=p, X=p, ld=p, st=p), **o))
    assert chol(D=0) == PM_EINVAL and chol(H=0) == PM_EINVAL and chol(H=1 << 31) == PM_ERANGE
    for k in ("S", "L", "X", "ld", "st"):
        assert chol(**{k: None}) == PM_EINVAL
    assert not any(keep)
