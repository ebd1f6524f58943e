"""Per-entry noise weights without a GPU: the NumPy restatement the GPU tests compare against
(tests/weighted_reference.py) pinned three ways -- omega = 1 is the masked reference at an all-ones mask, omega in {0, 1} is
the masked reference, omega = c is the all-ones reference at sigma / sqrt(c) --; the new C-ABI entries exist and reject bad
arguments before they touch a device; the host refusals, none of which needs a device or records a launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import masked_reference as MR
import recon_reference as R
import weighted_reference as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pm_weighted_prepare_f64", "pm_bsc_weighted_estep_f64", "pm_mca_weighted_select_scores_f64",
       "pm_mca_weighted_estep_f64")
PM_EINVAL, PM_ERANGE = -1, -2
KINDS = ["bsc", "mca", "mmca"]


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


# ------------------------------------------------------------------------------------------------ the reference, pinned
@pytest.mark.parametrize("kind", KINDS)
def test_unit_weights_are_the_masked_reference_at_an_all_ones_mask(kind):
    p, Y, _ = _case(kind, 31)
    ones = np.ones(Y.shape)
    yhat, ll, var = WR.enumerate_all(kind, p, Y, ones)
    want_y, want_l = MR.enumerate_all(kind, p, Y, ones.astype(bool))
    assert R.row_rel_err(yhat, want_y) < 1e-13
    np.testing.assert_allclose(ll, want_l, rtol=1e-13, atol=1e-13)
    assert (var >= 0).all()
    for Hp in (2, 5):
        np.testing.assert_array_equal(WR.select(kind, p, Y, ones, Hp), MR.model_terms(kind, p)[1](Y, ones.astype(bool), Hp))


@pytest.mark.parametrize("kind", KINDS)
def test_zero_one_weights_are_the_masked_reference(kind):
    """The unobserved entries of y hold NaN: they are never read.  Rows of all ones and all zeros, one dimension zero in
    every row."""
    from prosper_amd.em.camodels import generate_state_matrix
    p, Y, rng = _case(kind, 32)
    M = rng.uniform(size=Y.shape) < 0.6
    M[0], M[1], M[:, 4] = True, False, False
    Yg = np.where(M, Y, np.nan)
    yhat, ll, var = WR.enumerate_all(kind, p, Yg, M.astype(np.float64))
    want_y, want_l = MR.enumerate_all(kind, p, Yg, M)
    assert np.isfinite(yhat).all() and np.isfinite(var).all()
    assert R.row_rel_err(yhat, want_y) < 1e-13
    np.testing.assert_allclose(ll, want_l, rtol=1e-13, atol=1e-13)
    assert abs(ll[1]) < 1e-12                   # nothing observed: log sum_s p(s) = 0
    sc, largest = WR.model_scores(kind, p, Yg, M.astype(np.float64))
    want_sc, want_largest = MR.model_scores(kind, p, Yg, M)
    assert largest == want_largest
    np.testing.assert_allclose(sc, want_sc, rtol=1e-14, atol=1e-300)
    cand = WR.select(kind, p, Yg, M.astype(np.float64), 3)
    np.testing.assert_array_equal(cand, MR.model_terms(kind, p)[1](Yg, M, 3))
    if kind == "bsc":
        np.testing.assert_array_equal(cand[1], [2, 3, 4])      # a row of zero weights: the H' largest indices
    SM = generate_state_matrix(3, 2)[2]
    a = WR.from_candidates(kind, p, Yg, M.astype(np.float64), cand, SM)
    b = MR.from_candidates(kind, p, Yg, M, cand, SM)
    assert R.row_rel_err(a[0], b[0]) < 1e-13
    np.testing.assert_allclose(a[1], b[1], rtol=1e-13)


@pytest.mark.parametrize("c", [0.37, 5.0])
@pytest.mark.parametrize("kind", KINDS)
def test_constant_weights_are_the_unweighted_model_at_sigma_over_sqrt_c(kind, c):
    """omega = c everywhere: noise variance sigma^2 / c in every entry.  The constant matches too:
    -D/2 log(2 pi sigma^2) + D/2 log c = -D/2 log(2 pi sigma^2 / c)."""
    p, Y, _ = _case(kind, 33)
    yhat, ll, var = WR.enumerate_all(kind, p, Y, np.full(Y.shape, c))
    q = dict(p, sigma=p["sigma"] / np.sqrt(c))
    want_y, want_l, want_v = WR.enumerate_all(kind, q, Y, np.ones(Y.shape))
    ref_y, ref_l = MR.enumerate_all(kind, q, Y, np.ones(Y.shape, dtype=bool))
    assert R.row_rel_err(yhat, want_y) < 1e-12 and R.row_rel_err(yhat, ref_y) < 1e-12
    np.testing.assert_allclose(ll, want_l, rtol=1e-12)
    np.testing.assert_allclose(ll, ref_l, rtol=1e-12)
    np.testing.assert_allclose(var, want_v, rtol=1e-9, atol=1e-12 * np.abs(want_y).max() ** 2)


def test_the_variance_is_the_second_moment_minus_the_squared_mean():
    p, Y, rng = _case("bsc", 34, N=6)
    Om = rng.uniform(0.25, 4, size=Y.shape) * (rng.uniform(size=Y.shape) > 0.3)
    H = p["W"].shape[1]
    yhat, ll, var = WR.enumerate_all("bsc", p, Y, Om)
    mean = WR.model_mean("bsc", p)
    states = WR.all_states(H)
    means = np.array([mean(s) for s in states])
    sizes = np.array([len(s) for s in states], dtype=np.float64)
    for n in range(Y.shape[0]):
        lj = WR.log_joints(Y[n], Om[n], means, sizes, H, p["pi"], p["sigma"])
        q = np.exp(lj - lj.max())
        q /= q.sum()
        np.testing.assert_allclose(var[n], q @ means ** 2 - (q @ means) ** 2, rtol=1e-9, atol=1e-13)
        # the joint written out entry by entry
        k = 5
        s = states[k]
        on = Om[n] > 0
        want = len(s) * np.log(p["pi"]) + (H - len(s)) * np.log(1 - p["pi"]) \
            + sum(0.5 * np.log(Om[n, d] / (2 * np.pi * p["sigma"] ** 2)) - 0.5 * Om[n, d] * (Y[n, d] - means[k, d]) ** 2
                  / p["sigma"] ** 2 for d in range(Y.shape[1]) if on[d])
        np.testing.assert_allclose(lj[k], want, rtol=1e-13)


# ------------------------------------------------------------------------------------------------------------ the C ABI
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
    assert _lib.load().pm_version() >= 1030 and _lib.MIN_VERSION >= 1030


@pytest.mark.parametrize("det", [False, True])
def test_entries_reject_bad_arguments_without_a_device(det):
    """Every pointer below is host memory (or NULL): a launch would fault, a correct entry returns before one."""
    from prosper_amd import _lib
    lib = _lib.load(det)
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    P = _lib.EStepParams(0.1, -0.5, 1.0, 0.0)
    Q = _lib.McaParams(0.1, -0.5, 1.0, 1 / 21., 0.0)

    def prep(Y=p, ldy=10, wg=p, ldo=10, mu=None, N=4, D=10, Xw=p, ldxw=10, Om=p, ldom=10, X0=p, ldx0=10, xn=p, dn=p, lw=p):
        return lib.pm_weighted_prepare_f64(Y, ldy, wg, ldo, mu, N, D, Xw, ldxw, Om, ldom, X0, ldx0, xn, dn, lw, None)
    for k in ("Y", "wg", "Xw", "Om", "xn", "dn", "lw"):
        assert prep(**{k: None}) == PM_EINVAL, k
    assert prep(N=-1) == PM_EINVAL and prep(D=0) == PM_EINVAL
    for k in ("ldy", "ldo", "ldxw", "ldom", "ldx0"):
        assert prep(**{k: 9}) == PM_EINVAL, k
    assert prep(D=2 ** 31, ldy=2 ** 31, ldo=2 ** 31, ldxw=2 ** 31, ldom=2 ** 31, ldx0=2 ** 31) == PM_ERANGE
    assert prep(N=0) == 0 and prep(N=0, X0=None, ldx0=0) == 0

    def bsc(b=p, ldb=8, g=p, ldg=8, xn=p, wg=p, ldo=10, Wt=p, ldw=10, sm=p, S=3, par=C.byref(P), N=4, H=8, D=10, Hp=3,
            cand=p, logpj=p, ldl=12):
        return lib.pm_bsc_weighted_estep_f64(b, ldb, g, ldg, xn, wg, ldo, Wt, ldw, sm, S, par, N, H, D, Hp, cand, logpj, ldl,
                                             None)
    for k in ("b", "g", "xn", "wg", "Wt", "sm", "par", "cand", "logpj"):
        assert bsc(**{k: None}) == PM_EINVAL, k
    assert bsc(N=-1) == PM_EINVAL and bsc(S=-1) == PM_EINVAL and bsc(H=0) == PM_EINVAL and bsc(Hp=0) == PM_EINVAL
    for k, v in (("ldb", 7), ("ldg", 7), ("ldo", 9), ("ldw", 9), ("ldl", 11)):
        assert bsc(**{k: v}) == PM_EINVAL, k
    assert bsc(H=32, ldb=32, ldg=32, ldl=40, Hp=17) == PM_ERANGE            # H' <= 16
    assert bsc(Hp=9) == PM_ERANGE                                             # H' <= H
    assert bsc(H=1025, ldb=1025, ldg=1025, ldl=1030) == PM_ERANGE             # H <= PM_MAX_H
    assert bsc(S=65536, ldl=70000) == PM_ERANGE
    assert bsc(N=0) == 0

    def sel(Y=p, ldy=10, wg=p, ldo=10, W=p, ldw=10, Rr=p, ldr=8, N=4, H=8, D=10):
        return lib.pm_mca_weighted_select_scores_f64(Y, ldy, wg, ldo, W, ldw, Rr, ldr, N, H, D, None)
    for k in ("Y", "wg", "W", "Rr"):
        assert sel(**{k: None}) == PM_EINVAL, k
    assert sel(N=-1) == PM_EINVAL and sel(H=0) == PM_EINVAL and sel(D=0) == PM_EINVAL
    for k, v in (("ldy", 9), ("ldo", 9), ("ldw", 9), ("ldr", 7)):
        assert sel(**{k: v}) == PM_EINVAL, k
    assert sel(N=2 ** 40) == PM_ERANGE
    assert sel(N=0) == 0

    def mca(A=p, lds=8, wn=p, ldwn=8, xn=p, X0=p, ldx=10, wg=p, ldo=10, Wrho=p, cand=p, sm=p, S=3, par=C.byref(Q), N=4,
            H=8, D=10, Hp=3, logpj=p, ldl=12, lse1=p, lseb=p):
        return lib.pm_mca_weighted_estep_f64(A, lds, wn, ldwn, xn, X0, ldx, wg, ldo, Wrho, cand, sm, S, par, N, H, D, Hp,
                                             logpj, ldl, lse1, lseb, None)
    for k in ("A", "wn", "xn", "X0", "wg", "Wrho", "cand", "sm", "par", "logpj", "lse1", "lseb"):
        assert mca(**{k: None}) == PM_EINVAL, k
    assert mca(N=-1) == PM_EINVAL and mca(S=-1) == PM_EINVAL and mca(H=0) == PM_EINVAL
    for k, v in (("lds", 7), ("ldwn", 7), ("ldx", 9), ("ldo", 9), ("ldl", 11)):
        assert mca(**{k: v}) == PM_EINVAL, k
    assert mca(D=1025, ldx=1025, ldo=1025) == PM_ERANGE                       # D <= 1024 as pm_mca_estep_f64
    assert mca(H=32, lds=32, ldwn=32, ldl=40, Hp=17) == PM_ERANGE
    assert mca(N=0) == 0


# ------------------------------------------------------------------------------------------------------------ refusals
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


def _recorded(model):
    """The model's launch hook, wrapped to keep the names of the entry points that ran (mixtures launch through _lib.call)."""
    calls = []
    if hasattr(model, "_call"):
        orig = model._call
        model._call = lambda label, entry, *args: (calls.append(entry), orig(label, entry, *args))[1]
    return calls


def test_a_weight_is_refused_by_name_before_any_launch():
    """No device on this machine: a refusal that came after a launch (or after a look at the device) would raise HipError."""
    built, ca, mix = _models()
    y, w = np.zeros((3, 4)), np.ones((3, 4))
    for cls in ca + mix:
        model = cls(4, 4, 2, 2) if cls in ca else cls(4, 4)
        calls = _recorded(model)
        for call in (lambda: model.reconstruct({}, {'y': y, 'weight': w}),
                     lambda: model.reconstruct({}, {'y': y, 'weight': w}, variance=True),
                     lambda: model.log_likelihood({}, {'y': y, 'weight': w}),
                     lambda: model.log_likelihood({}, {'y': y, 'weight': w}, per_datapoint=True),
                     lambda: model.sample_posterior({}, {'y': y, 'weight': w}),
                     lambda: model.reconstruct_image({}, np.zeros((4, 4)), weight=np.ones((4, 4)), patch=2)):
            with pytest.raises(NotImplementedError, match="(?s)%s.*weight" % cls.__name__):
                call()
        assert not calls, (cls.__name__, calls)


def test_training_refuses_a_weight_by_name_for_every_model():
    built, ca, mix = _models()
    y, w = np.zeros((3, 4)), np.ones((3, 4))
    data = {'y': y, 'weight': w}
    for cls in built + ca + mix:
        model = cls(4, 4, 2, 2) if cls not in mix else cls(4, 4)
        calls = _recorded(model)
        todo = [lambda: model.step({}, {}, dict(data)), lambda: model.E_step({}, {}, dict(data)),
                lambda: model.M_step({}, {}, {}, dict(data))]
        if cls not in mix:
            todo.append(lambda: model.select_Hprimes({}, dict(data)))
        for call in todo:
            with pytest.raises(NotImplementedError, match="(?s)%s.*weight" % cls.__name__):
                call()
        assert not calls, (cls.__name__, calls)


def test_argument_errors_of_the_built_models_need_no_device():
    from prosper_amd import _lib
    from prosper_amd.utils.patches import denoise_image
    built, _, _ = _models()
    y = np.zeros((3, 4))
    ok = np.ones((3, 4))
    for cls in built:
        model = cls(4, 4, 2, 2)
        calls = _recorded(model)
        entries = (lambda d, **kw: model.reconstruct({}, d, **kw), lambda d, **kw: model.log_likelihood({}, d, **kw),
                   lambda d, **kw: model.sample_posterior({}, d, **kw))
        for bad in (np.ones((3, 5)), np.ones((4, 3)), np.ones(12), np.ones((3, 4, 1))):
            for f in entries:
                with pytest.raises(ValueError, match="weight"):
                    f({'y': y, 'weight': bad})
        for v in (-1.0, -1e-300, np.nan, np.inf, -np.inf):
            bad = ok.copy()
            bad[2, 1] = v
            for f in entries:
                with pytest.raises(ValueError, match="weight"):
                    f({'y': y, 'weight': bad})
            if np.float32(v) != 0:              # (-1e-300 rounds to -0.0 in float32, which is a zero weight)
                with pytest.raises(ValueError, match="weight"):
                    model.reconstruct({}, {'y': y, 'weight': bad.astype(np.float32)}, variance=True)
            img = np.ones((4, 4))
            img[1, 2] = v
            with pytest.raises(ValueError, match="weight"):
                model.reconstruct_image({}, np.zeros((4, 4)), weight=img, patch=2)
        for f in entries:
            with pytest.raises(ValueError, match="(?s)weight.*mask.*zeros"):
                f({'y': y, 'weight': ok, 'mask': np.ones((3, 4), dtype=bool)})
        for f in entries[:2]:
            with pytest.raises(NotImplementedError, match="(?s)exact.*weight"):
                f({'y': y, 'weight': ok}, exact=True)
        with pytest.raises(ValueError, match="center"):
            model.reconstruct_image({}, np.zeros((4, 4)), weight=np.ones((4, 4)), center=True, patch=2)
        with pytest.raises(ValueError, match="(?s)weight.*mask"):
            model.reconstruct_image({}, np.zeros((4, 4)), weight=np.ones((4, 4)), mask=np.ones((4, 4)), patch=2)
        with pytest.raises(ValueError, match="weight"):
            model.reconstruct_image({}, np.zeros((4, 4)), weight=np.ones((4, 5)), patch=2)
        with pytest.raises(NotImplementedError, match="exact"):
            model.reconstruct_image({}, np.zeros((4, 4)), weight=np.ones((4, 4)), exact=True, patch=2)
        with pytest.raises(ValueError, match="center"):
            denoise_image(model, {}, np.zeros((4, 4)), weight=np.ones((4, 4)), center=True, patch=2)
        assert not calls, (cls.__name__, calls)
        big = cls(4, 20, 17, 2)
        calls = _recorded(big)
        for f in (lambda: big.reconstruct({}, {'y': y, 'weight': ok}), lambda: big.log_likelihood({}, {'y': y, 'weight': ok}),
                  lambda: big.sample_posterior({}, {'y': y, 'weight': ok})):
            with pytest.raises(_lib.HipError, match="16"):
                f()
        assert not calls, (cls.__name__, calls)


def test_the_signatures_of_the_inference_methods_did_not_move():
    import inspect
    built, ca, mix = _models()
    for cls in built + ca:
        assert list(inspect.signature(cls.reconstruct).parameters) == ["self", "model_params", "my_data", "device", "exact",
                                                                       "variance"]
        assert list(inspect.signature(cls.log_likelihood).parameters) == ["self", "model_params", "my_data", "per_datapoint",
                                                                          "exact"]
    for cls in built + ca + mix:
        par = inspect.signature(cls.reconstruct_image).parameters
        assert "weight" in par and par["weight"].default is None
    from prosper_amd.utils.patches import denoise_image
    par = inspect.signature(denoise_image).parameters
    assert list(par)[-1] == "weight" and par["weight"].default is None
