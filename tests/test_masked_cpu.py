"""Missing values without a GPU: the NumPy restatement the GPU tests compare against
(tests/masked_reference.py) agrees with recon_reference at an all-ones mask and with the unmasked enumeration of the
sub-model; the new C-ABI entries exist and reject bad arguments before they touch a device; the host refusals that need no
device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy.special import logsumexp

import masked_reference as MR
import recon_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pm_masked_prepare_f64", "pm_bsc_masked_estep_f64", "pm_mca_masked_select_scores_f64", "pm_mca_masked_estep_f64")
PM_EINVAL, PM_ERANGE = -1, -2


def _case(kind, seed, D=9, H=5, N=40):
    rng = np.random.RandomState(seed)
    if kind == "bsc":
        p = {"W": rng.normal(size=(D, H)), "pi": 0.3, "sigma": 0.9, "mu": rng.normal(size=D)}
        Y = (rng.uniform(size=(N, H)) < 0.3) @ p["W"].T + p["mu"] + 0.9 * rng.normal(size=(N, D))
    else:
        W = rng.uniform(0.2, 3.0, size=(D, H))
        if kind == "mmca":
            W *= rng.choice([-1.0, 1.0], size=(D, H))
        p = {"W": W, "pi": 0.3, "sigma": 0.7}
        Y = rng.uniform(-1 if kind == "mmca" else 0, 3, size=(N, D))
    return p, Y, rng


def _plain_loglik(kind, p, Y):
    """log sum_s p(s, y) of the unmasked model, written out independently of masked_reference.evaluate."""
    W = p["W"]
    D, H = W.shape
    mean, _ = MR.model_terms(kind, p)
    states = MR.all_states(H)
    means = np.array([mean(s) for s in states])
    k = np.array([len(s) for s in states])
    lj = k * np.log(p["pi"]) + (H - k) * np.log(1 - p["pi"]) - 0.5 * D * np.log(2 * np.pi * p["sigma"] ** 2) \
        - 0.5 * ((Y[:, None, :] - means[None]) ** 2).sum(-1) / p["sigma"] ** 2
    return logsumexp(lj, axis=1)


@pytest.mark.parametrize("kind", ["bsc", "mca", "mmca"])
def test_all_ones_mask_is_the_unmasked_enumeration(kind):
    p, Y, _ = _case(kind, 11)
    yhat, ll = MR.enumerate_all(kind, p, Y, np.ones(Y.shape, dtype=bool))
    if kind == "bsc":
        want = R.enum_linear(Y, p["W"], p["sigma"], [0., 1.], np.log([1 - p["pi"], p["pi"]]), mu=p["mu"])
    else:
        want = R.enum_mca(Y, p["W"], 21.0 if kind == "mca" else 6.0, kind == "mmca", p["pi"], p["sigma"])
    assert R.row_rel_err(yhat, want) < 1e-12
    np.testing.assert_allclose(ll, _plain_loglik(kind, p, Y), rtol=1e-13, atol=1e-12)


@pytest.mark.parametrize("kind", ["bsc", "mca", "mmca"])
def test_shared_mask_is_the_sub_model(kind):
    """One mask for all rows: deleting the masked rows of W (and mu) and the masked columns of y gives an unmasked model
    whose enumeration is the masked one's -- the log-likelihood, and the observed dimensions of the posterior mean.  The
    unobserved entries of y hold NaN: they are never read."""
    p, Y, rng = _case(kind, 12)
    obs = rng.uniform(size=Y.shape[1]) < 0.6
    assert 0 < obs.sum() < obs.size
    M = np.tile(obs, (Y.shape[0], 1))
    Yg = np.where(M, Y, np.nan)
    yhat, ll = MR.enumerate_all(kind, p, Yg, M)
    sub = dict(p, W=p["W"][obs])
    if "mu" in p:
        sub["mu"] = p["mu"][obs]
    if kind == "bsc":
        want = R.enum_linear(Y[:, obs], sub["W"], p["sigma"], [0., 1.], np.log([1 - p["pi"], p["pi"]]), mu=sub["mu"])
    else:
        want = R.enum_mca(Y[:, obs], sub["W"], 21.0 if kind == "mca" else 6.0, kind == "mmca", p["pi"], p["sigma"])
    assert np.isfinite(yhat).all()
    assert R.row_rel_err(yhat[:, obs], want) < 1e-12
    np.testing.assert_allclose(ll, _plain_loglik(kind, sub, Y[:, obs]), rtol=1e-13, atol=1e-12)


def test_truncated_sums_at_the_full_candidate_set_are_the_enumeration():
    """from_candidates with H' = gamma = H rebuilds exactly the enumeration (column layout, candidate scatter); an empty row
    of the mask gives the prior and the H' largest indices."""
    from prosper_amd.em.camodels import generate_state_matrix
    for kind in ("bsc", "mca", "mmca"):
        p, Y, rng = _case(kind, 13, N=12)
        H = p["W"].shape[1]
        M = rng.uniform(size=Y.shape) < 0.5
        M[0], M[1] = True, False
        SM = generate_state_matrix(H, H)[2]
        _, sel = MR.model_terms(kind, p)
        cand = sel(Y, M, H)
        assert sorted(cand[3]) == list(range(H))
        a = MR.from_candidates(kind, p, Y, M, cand, SM)
        b = MR.enumerate_all(kind, p, Y, M)
        assert R.row_rel_err(a[0], b[0]) < 1e-12
        np.testing.assert_allclose(a[1], b[1], rtol=1e-13)
        # nothing observed: log sum_s p(s) = 0 and the posterior is the prior
        assert abs(b[1][1]) < 1e-12
    p, Y, _ = _case("bsc", 14)
    M = np.zeros(Y.shape, dtype=bool)
    assert np.array_equal(MR.select_bsc(Y, M, p["W"], 3, p["mu"])[0], [2, 3, 4])


def test_boundary_gap_of_the_selection_scores():
    """The distance between the last score selected and the first left out, in the ranking's direction; 0 for a tie."""
    sc = np.array([[5., 1., 4., 2., 3.], [1., 2., 2., 0., 7.], [0., 0., 0., 0., 0.], [-4., -2., 8., -1., 6.]])
    np.testing.assert_allclose(MR.boundary_gap(sc, 2, True), [0.25, 0.0, 0.0, 7. / 6.])        # 4|3, 2|2, 0|0, 6|-1
    np.testing.assert_allclose(MR.boundary_gap(sc, 2, False), [1. / 3., 0.5, 0.0, 0.5])        # 2|3, 1|2, 0|0, -2|-1
    assert np.isinf(MR.boundary_gap(sc, 5, True)).all() and np.isinf(MR.boundary_gap(sc, 5, False)).all()
    # ... and the scores are the ones the selections rank
    for kind in ("bsc", "mca", "mmca"):
        p, Y, rng = _case(kind, 15, H=7)
        M = rng.uniform(size=Y.shape) < 0.6
        sc, largest = MR.model_scores(kind, p, Y, M)
        _, sel = MR.model_terms(kind, p)
        cand = sel(Y, M, 3)
        rest = np.array([np.setdiff1d(np.arange(7), c) for c in cand])
        picked, left = np.take_along_axis(sc, cand, 1), np.take_along_axis(sc, rest, 1)
        assert ((picked.min(1) >= left.max(1)) if largest else (picked.max(1) <= left.min(1))).all()
        edge = np.abs(picked.min(1) - left.max(1)) if largest else np.abs(left.min(1) - picked.max(1))
        scale = np.maximum(np.abs(picked.min(1) if largest else picked.max(1)), np.abs(left.max(1) if largest else left.min(1)))
        np.testing.assert_allclose(MR.boundary_gap(sc, 3, largest), edge / scale, rtol=1e-14)


def test_bsc_selection_rule_on_ties_nan_and_infinities():
    inf, nan = np.inf, np.nan
    b = np.array([[6., 9., 1., 0., 7., 0.],            # 6/2 == 9/3: the larger index of the tie is nearer the top
                  [nan, 5., nan, 1., 2., 3.],          # NaN ranks lowest
                  [-inf, -inf, 1., -inf, -inf, -inf],  # -inf fills from the largest index
                  [nan, nan, nan, nan, nan, nan]])
    g = np.array([[4., 9., 1., 0., 0., 4.], [1.] * 6, [1.] * 6, [1.] * 6])
    assert np.array_equal(MR.bsc_select_rule(b, g, 2), [[0, 1], [5, 1], [5, 2], [4, 5]])
    assert np.array_equal(MR.bsc_select_rule(b, g, 5)[0], [4, 5, 2, 0, 1])     # of the three zeros (g = 0 twice, b = 0) the larger indices
    assert np.array_equal(MR.bsc_select_rule(b, g, 3)[1], [4, 5, 1])
    assert np.array_equal(MR.bsc_select_rule(b, g, 6)[1], [0, 2, 3, 4, 5, 1])
    # on continuous data it is select_bsc
    p, Y, rng = _case("bsc", 16, H=7)
    M = rng.uniform(size=Y.shape) < 0.6
    X = np.where(M, Y - p["mu"], 0.0)
    assert np.array_equal(MR.bsc_select_rule(X @ p["W"], M.astype(float) @ p["W"] ** 2, 3), MR.select_bsc(Y, M, p["W"], 3, p["mu"]))


def test_bsc_masked_terms_are_the_masked_energies():
    """Integer data: e_s of bsc_masked_terms equals sum_d m_d (x_d - sum_{h in s} W_dh)^2 written out state by state,
    exactly, and |s| is the state's size; with continuous data the columns are the log-joints ``evaluate`` sums."""
    from prosper_amd.em.camodels import generate_state_matrix
    rng = np.random.RandomState(17)
    N, D, H, Hp = 6, 11, 9, 4
    SM = generate_state_matrix(Hp, 3)[2]
    Wt = rng.randint(-3, 4, size=(H, D)).astype(np.float64)
    X = rng.randint(-8, 9, size=(N, D)).astype(np.float64)
    M = rng.uniform(size=(N, D)) < 0.6
    M[1] = False
    X0, Mf = np.where(M, X, 0.0), M.astype(np.float64)
    b, g, xn2 = X0 @ Wt.T, Mf @ (Wt * Wt).T, (X0 * X0).sum(1)
    cand = MR.bsc_select_rule(b, g, Hp)
    size, e = MR.bsc_masked_terms(b, g, xn2, M, Wt, cand, SM)
    for n in range(N):
        states = MR.truncated_states(H, cand[n], SM)
        assert len(states) == e.shape[1]
        for k, s in enumerate(states):
            assert size[n, k] == len(s)
            assert e[n, k] == (Mf[n] * (X[n] - Wt[list(s)].sum(axis=0)) ** 2).sum(), (n, k)
    pi, sigma = 0.2, 1.1
    _, ll = MR.evaluate(X, M, [MR.truncated_states(H, c, SM) for c in cand], MR.bsc_mean(Wt.T), H, pi, sigma)
    lj = np.log(pi / (1 - pi)) * size - 0.5 / sigma ** 2 * e
    want = logsumexp(lj, axis=1) + H * np.log(1 - pi) - 0.5 * M.sum(1) * np.log(2 * np.pi * sigma ** 2)
    np.testing.assert_allclose(ll, want, rtol=1e-13)


def test_new_entries_in_header_binding_and_both_libraries():
    from prosper_amd import _lib
    header = open(os.path.join(ROOT, "include", "prosper_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    for path in (_lib.LIB_PATH, _lib.LIB_PATH_DET):
        lib = C.CDLL(path)
        for name in NEW:
            assert hasattr(lib, name), (path, name)
    assert _lib.load().pm_version() >= 1021 and _lib.MIN_VERSION >= 1021


@pytest.mark.parametrize("det", [False, True])
def test_entries_reject_bad_arguments_without_a_device(det):
    """Every pointer below is host memory (or NULL): a launch would fault, a correct entry returns before one."""
    from prosper_amd import _lib
    lib = _lib.load(det)
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    P = _lib.EStepParams(0.1, -0.5, 1.0, 0.0)
    Q = _lib.McaParams(0.1, -0.5, 1.0, 1 / 21., 0.0)

    def prep(Y=p, ldy=10, mask=p, ldm=10, mu=None, N=4, D=10, X0=p, ldx=10, Mf=p, ldf=10, xn=p, dn=p):
        return lib.pm_masked_prepare_f64(Y, ldy, mask, ldm, mu, N, D, X0, ldx, Mf, ldf, xn, dn, None)
    for k in ("Y", "mask", "X0", "xn", "dn"):
        assert prep(**{k: None}) == PM_EINVAL, k
    assert prep(N=-1) == PM_EINVAL and prep(D=0) == PM_EINVAL
    for k in ("ldy", "ldm", "ldx", "ldf"):
        assert prep(**{k: 9}) == PM_EINVAL, k
    assert prep(D=2 ** 31, ldy=2 ** 31, ldm=2 ** 31, ldx=2 ** 31, ldf=2 ** 31) == PM_ERANGE
    assert prep(N=0) == 0

    def bsc(b=p, ldb=8, g=p, ldg=8, xn=p, mask=p, ldm=10, Wt=p, ldw=10, sm=p, S=3, par=C.byref(P), N=4, H=8, D=10, Hp=3,
            cand=p, logpj=p, ldl=12):
        return lib.pm_bsc_masked_estep_f64(b, ldb, g, ldg, xn, mask, ldm, Wt, ldw, sm, S, par, N, H, D, Hp, cand, logpj, ldl,
                                           None)
    for k in ("b", "g", "xn", "mask", "Wt", "sm", "par", "cand", "logpj"):
        assert bsc(**{k: None}) == PM_EINVAL, k
    assert bsc(N=-1) == PM_EINVAL and bsc(S=-1) == PM_EINVAL and bsc(H=0) == PM_EINVAL and bsc(Hp=0) == PM_EINVAL
    for k, v in (("ldb", 7), ("ldg", 7), ("ldm", 9), ("ldw", 9), ("ldl", 11)):
        assert bsc(**{k: v}) == PM_EINVAL, k
    assert bsc(H=32, ldb=32, ldg=32, ldl=40, Hp=17) == PM_ERANGE            # H' <= 16
    assert bsc(Hp=9) == PM_ERANGE                                             # H' <= H
    assert bsc(H=1025, ldb=1025, ldg=1025, ldl=1030) == PM_ERANGE             # the H range of the general kernels
    assert bsc(S=65536, ldl=70000) == PM_ERANGE
    assert bsc(N=0) == 0

    def sel(Y=p, ldy=10, mask=p, ldm=10, W=p, ldw=10, Rr=p, ldr=8, N=4, H=8, D=10):
        return lib.pm_mca_masked_select_scores_f64(Y, ldy, mask, ldm, W, ldw, Rr, ldr, N, H, D, None)
    for k in ("Y", "mask", "W", "Rr"):
        assert sel(**{k: None}) == PM_EINVAL, k
    assert sel(N=-1) == PM_EINVAL and sel(H=0) == PM_EINVAL and sel(D=0) == PM_EINVAL
    for k, v in (("ldy", 9), ("ldm", 9), ("ldw", 9), ("ldr", 7)):
        assert sel(**{k: v}) == PM_EINVAL, k
    assert sel(N=2 ** 40) == PM_ERANGE
    assert sel(N=0) == 0

    def mca(A=p, lds=8, wn=p, ldwn=8, xn=p, X0=p, ldx=10, mask=p, ldm=10, Wrho=p, cand=p, sm=p, S=3, par=C.byref(Q), N=4,
            H=8, D=10, Hp=3, logpj=p, ldl=12, lse1=p, lseb=p):
        return lib.pm_mca_masked_estep_f64(A, lds, wn, ldwn, xn, X0, ldx, mask, ldm, Wrho, cand, sm, S, par, N, H, D, Hp,
                                           logpj, ldl, lse1, lseb, None)
    for k in ("A", "wn", "xn", "X0", "mask", "Wrho", "cand", "sm", "par", "logpj", "lse1", "lseb"):
        assert mca(**{k: None}) == PM_EINVAL, k
    assert mca(N=-1) == PM_EINVAL and mca(S=-1) == PM_EINVAL and mca(H=0) == PM_EINVAL
    for k, v in (("lds", 7), ("ldwn", 7), ("ldx", 9), ("ldm", 9), ("ldl", 11)):
        assert mca(**{k: v}) == PM_EINVAL, k
    assert mca(D=1025, ldx=1025, ldm=1025) == PM_ERANGE                       # D <= 1024 as pm_mca_estep_f64
    assert mca(H=32, lds=32, ldwn=32, ldl=40, Hp=17) == PM_ERANGE
    assert mca(N=0) == 0


def _models():
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    from prosper_amd.em.camodels.mmca_et import MMCA_ET
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    from prosper_amd.em.camodels.tsc_et import TSC_ET
    from prosper_amd.em.camodels.gsc_et import GSC
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.em.mixturemodels.MoP import MoP
    return (BSC_ET, MCA_ET, MMCA_ET), (DSC_ET, TSC_ET, GSC), (MoG, MoP)


def test_a_mask_is_refused_by_name_before_any_launch():
    """No device on this machine: a refusal that came after a launch (or after a look at the device) would raise HipError."""
    built, ca, mix = _models()
    y, m = np.zeros((3, 4)), np.ones((3, 4), dtype=bool)
    for cls in ca:
        model = cls(4, 4, 2, 2)
        for call in (lambda: model.reconstruct({}, {'y': y, 'mask': m}),
                     lambda: model.log_likelihood({}, {'y': y, 'mask': m}),
                     lambda: model.reconstruct_image({}, np.zeros((4, 4)), mask=np.ones((4, 4)), center=True)):
            with pytest.raises((NotImplementedError, ValueError), match=cls.__name__ + "|center"):
                call()
        with pytest.raises(NotImplementedError, match=cls.__name__):
            model.reconstruct({}, {'y': y, 'mask': m})
    for cls in mix:
        model = cls(4, 4)
        with pytest.raises(NotImplementedError, match=cls.__name__):
            model.reconstruct({}, {'y': y, 'mask': m})
        with pytest.raises(NotImplementedError, match=cls.__name__):
            model.log_likelihood({}, {'y': y, 'mask': m}, per_datapoint=True)


def test_argument_errors_of_the_built_models_need_no_device():
    built, _, _ = _models()
    y = np.zeros((3, 4))
    for cls in built:
        model = cls(4, 4, 2, 2)
        for bad in (np.ones((3, 5)), np.ones((4, 3)), np.ones(12), np.ones((3, 4, 1))):
            with pytest.raises(ValueError, match="mask"):
                model.reconstruct({}, {'y': y, 'mask': bad})
            with pytest.raises(ValueError, match="mask"):
                model.log_likelihood({}, {'y': y, 'mask': bad})
        with pytest.raises(NotImplementedError, match="exact"):
            model.log_likelihood({}, {'y': y, 'mask': np.ones((3, 4))}, exact=True)
        with pytest.raises(ValueError, match="center"):
            model.reconstruct_image({}, np.zeros((4, 4)), mask=np.ones((4, 4)), center=True)
    from prosper_amd.utils.patches import denoise_image
    with pytest.raises(ValueError, match="center"):
        denoise_image(built[0](4, 4, 2, 2), {}, np.zeros((4, 4)), mask=np.ones((4, 4)), center=True)
