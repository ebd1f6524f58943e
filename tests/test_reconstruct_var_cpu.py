"""reconstruct(variance=True) without a GPU: the keyword and the new C-ABI entries exist in the signatures, the
header, the binding and both libraries; the refusals come before anything touches a device; the entries reject bad arguments
before a launch; the two forms of V in tests/recon_var_reference.py agree; and the calibration identity holds on the
reference alone."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import recon_reference as R
import recon_var_reference as RV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pm_recon_moments2_f64", "pm_recon_gsc_moments2_f64", "pm_recon_var_finish_f64", "pm_recon_mca_var_f64")
PM_EINVAL, PM_ERANGE = -1, -2


def _models():
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    from prosper_amd.em.camodels.mmca_et import MMCA_ET
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    from prosper_amd.em.camodels.tsc_et import TSC_ET
    from prosper_amd.em.camodels.gsc_et import GSC
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.em.mixturemodels.MoP import MoP
    return (BSC_ET, MCA_ET, MMCA_ET, DSC_ET, TSC_ET, GSC), (MoG, MoP)


def test_every_model_and_the_image_path_take_variance():
    from prosper_amd.utils import patches
    ca, mix = _models()
    for cls in ca + mix:
        par = inspect.signature(cls.reconstruct).parameters
        assert list(par)[:6] == ["self", "model_params", "my_data", "device", "exact", "variance"], cls.__name__
        assert par["variance"].default is False
        doc = cls.reconstruct.__doc__
        assert "variance=True" in doc and "NOISELESS" in doc and "caller adds" in doc, cls.__name__
        assert "variance" in cls.reconstruct_image.__doc__
    par = inspect.signature(patches.denoise_image).parameters
    assert par["variance"].default is False
    assert "upper bound" in patches.denoise_image.__doc__


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
    assert _lib.load().pm_version() >= 1026 and _lib.MIN_VERSION >= 1026
    assert _lib.load(True).pm_version() >= _lib.MIN_VERSION


# ------------------------------------------------------------------------------------------- refusals before any launch
def test_exact_with_variance_is_refused_by_name():
    """No device on this machine: a refusal that came after a look at the device would raise HipError."""
    ca, mix = _models()
    y = np.zeros((3, 4))
    for model in [cls(4, 4, 2, 2) for cls in ca] + [cls(4, 4) for cls in mix]:
        with pytest.raises(NotImplementedError, match="variance"):
            model.reconstruct({}, {'y': y}, exact=True, variance=True)
        with pytest.raises(NotImplementedError, match="variance"):
            model.reconstruct_image({}, np.zeros((4, 4)), patch=2, exact=True, variance=True)


def test_a_mask_on_the_other_models_keeps_its_refusal():
    ca, mix = _models()
    y, m = np.zeros((3, 4)), np.ones((3, 4), dtype=bool)
    for model in [cls(4, 4, 2, 2) for cls in ca[3:]] + [cls(4, 4) for cls in mix]:
        with pytest.raises(NotImplementedError, match=type(model).__name__ + r".*mask"):
            model.reconstruct({}, {'y': y, 'mask': m}, variance=True)
    for cls in ca[:3]:
        with pytest.raises(NotImplementedError, match="exact=True with a mask"):
            cls(4, 4, 2, 2).reconstruct({}, {'y': y, 'mask': m}, exact=True, variance=True)


def test_more_than_sixteen_candidates_are_refused():
    """The constructors take H' = 17; the refusal is ``reconstruct(variance=True)``'s own, by name, with no device here.  MCA /
    MMCA also refuse D = 1025 there."""
    from prosper_amd import _lib
    ca, _ = _models()
    for cls in ca[:5]:
        model = cls(4, 40, 17, 2)
        assert model.Hprime == 17
        with pytest.raises(_lib.HipError, match="variance=True holds H' <= 16"):
            model.reconstruct({}, {'y': np.zeros((3, 4))}, variance=True)
    for cls in ca[1:3]:
        with pytest.raises(_lib.HipError, match="variance=True holds D <= 1024"):
            cls(1025, 8, 4, 2).reconstruct({}, {'y': np.zeros((3, 1025))}, variance=True)


def test_image_path_refuses_exact_with_variance_after_the_mask_refusals():
    ca, _ = _models()
    img, mask = np.zeros((4, 4)), np.ones((4, 4))
    with pytest.raises(NotImplementedError, match="exact=True with a mask"):
        ca[0](4, 4, 2, 2).reconstruct_image({}, img, patch=2, mask=mask, exact=True, variance=True)
    with pytest.raises(NotImplementedError, match="DSC_ET.*mask"):
        ca[3](4, 4, 2, 2).reconstruct_image({}, img, patch=2, mask=mask, exact=True, variance=True)


def test_no_rows_give_two_empty_arrays():
    ca, mix = _models()
    for model in [cls(4, 4, 2, 2) for cls in ca] + [cls(4, 4) for cls in mix]:
        out = model.reconstruct({}, {'y': np.zeros((0, 4))}, variance=True)
        assert isinstance(out, tuple) and len(out) == 2
        assert all(o.shape == (0, 4) and o.dtype == np.float64 for o in out)


# ---------------------------------------------------------------------------------------------------- argument checks
@pytest.mark.parametrize("det", [False, True])
def test_entries_reject_bad_arguments_without_a_device(det):
    """Every pointer below is host memory (or NULL): a launch would fault, a correct entry returns before one."""
    from prosper_amd import _lib
    lib = _lib.load(det)
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    one = (C.c_double * 8)(1.0)

    def mom(logpj=p, ld=10, lse=None, a=1.0, off=None, cand=p, vals=p, bv=one, N=4, H=4, Hp=3, K=9, soff=1, nblk=1, moff=5,
            S=4, m2=p, ldm=8, cols=8, pp=p, ldp=3):
        return lib.pm_recon_moments2_f64(logpj, ld, lse, a, off, cand, vals, bv, N, H, Hp, K, soff, nblk, moff, S, m2, ldm, cols,
                                         pp, ldp, None)
    for k in ("logpj", "cand", "vals", "bv", "m2", "pp"):
        assert mom(**{k: None}) == PM_EINVAL, k
        assert mom(N=0, **{k: None}) == PM_EINVAL, k                    # null pointers are refused at N = 0 too
    assert mom(N=-1) == PM_EINVAL and mom(H=0) == PM_EINVAL and mom(ld=8) == PM_EINVAL and mom(S=-1) == PM_EINVAL
    assert mom(ldm=7) == PM_EINVAL and mom(cols=3) == PM_EINVAL and mom(ldp=2) == PM_EINVAL
    assert mom(moff=6) == PM_EINVAL and mom(nblk=3) == PM_EINVAL          # columns past K
    assert mom(lse=p, a=0.5) == PM_EINVAL and mom(lse=p, off=p) == PM_EINVAL
    assert mom(Hp=0) == PM_EINVAL                                         # table states without candidates
    assert mom(Hp=17, ldp=200) == PM_ERANGE and mom(nblk=9, K=200, ld=200) == PM_ERANGE
    assert mom(N=0) == 0
    assert mom(N=0, Hp=1, pp=None) == 0 and mom(N=0, S=0, moff=0, cand=None, vals=None, pp=None) == 0   # no pairs: p may be NULL

    def gsc(lp=p, ldl=12, blk=p, ldb=25, sc=p, lds=4, tab=p, cand=p, beta=0.5, N=4, H=4, Hp=3, S=4, m2=p, ldm=8, cols=8, pp=p,
            ldp=3):
        return lib.pm_recon_gsc_moments2_f64(lp, ldl, blk, ldb, sc, lds, tab, cand, beta, N, H, Hp, S, m2, ldm, cols, pp, ldp,
                                             None)
    for k in ("lp", "sc", "tab", "cand", "m2", "pp"):
        assert gsc(**{k: None}) == PM_EINVAL, k
        assert gsc(N=0, **{k: None}) == PM_EINVAL, k
    assert gsc(N=-1) == PM_EINVAL and gsc(H=0) == PM_EINVAL and gsc(Hp=0) == PM_EINVAL and gsc(ldl=8) == PM_EINVAL
    assert gsc(ldb=24) == PM_EINVAL and gsc(lds=3) == PM_EINVAL and gsc(ldm=7) == PM_EINVAL and gsc(cols=3) == PM_EINVAL
    assert gsc(ldp=2) == PM_EINVAL and gsc(beta=0.0) == PM_EINVAL
    assert gsc(Hp=17, ldb=700, ldp=200) == PM_ERANGE
    assert gsc(N=0) == 0 and gsc(N=0, blk=None, cand=None, pp=None, S=0, ldl=5) == 0

    def fin(V=p, ldv=10, Y=p, ldy=10, mu=None, pp=p, ldp=3, cand=p, Wt=p, ldw=10, N=4, H=4, D=10, Hp=3):
        return lib.pm_recon_var_finish_f64(V, ldv, Y, ldy, mu, pp, ldp, cand, Wt, ldw, N, H, D, Hp, None)
    for k in ("V", "Y", "cand", "Wt"):
        assert fin(**{k: None}) == PM_EINVAL, k
        assert fin(N=0, **{k: None}) == PM_EINVAL, k
    assert fin(N=-1) == PM_EINVAL and fin(H=0) == PM_EINVAL and fin(D=0) == PM_EINVAL and fin(Hp=-1) == PM_EINVAL
    assert fin(ldv=9) == PM_EINVAL and fin(ldy=9) == PM_EINVAL and fin(ldw=9) == PM_EINVAL and fin(ldp=2) == PM_EINVAL
    assert fin(Hp=17, ldp=200) == PM_ERANGE
    assert fin(N=0) == 0 and fin(N=0, mu=p) == 0
    assert fin(N=0, pp=None, cand=None, Wt=None, Hp=0) == 0 and fin(N=0, cand=None, Wt=None, Hp=1) == 0   # no pairs

    def mca(logpj=p, ld=100, cand=p, masks=p, Wrho=p, inv_rho=1 / 21., N=4, H=4, D=10, Hp=2, S=1, V=p, ldv=None):
        return lib.pm_recon_mca_var_f64(logpj, ld, None, cand, masks, Wrho, inv_rho, 0, N, H, D, Hp, S, V,
                                        D if ldv is None else ldv, None)
    for k in ("logpj", "cand", "masks", "Wrho", "V"):
        assert mca(**{k: None}) == PM_EINVAL, k
        assert mca(N=0, **{k: None}) == PM_EINVAL, k
    assert mca(N=-1) == PM_EINVAL and mca(ld=5) == PM_EINVAL and mca(ldv=9) == PM_EINVAL and mca(inv_rho=0.0) == PM_EINVAL
    assert mca(D=1025, ldv=1025) == PM_ERANGE and mca(Hp=17) == PM_ERANGE
    assert mca(N=0) == 0 and mca(S=0) == 0


# ------------------------------------------------------------------------------------------------- the reference itself
def _close(ref, tol=1e-13):
    scale = np.abs(ref.E2).max(axis=1)
    return float((np.abs(ref.V - (ref.E2 - ref.yhat ** 2)).max(axis=1) / scale).max()) <= tol


def test_the_two_forms_of_v_agree_for_every_model():
    rng = np.random.RandomState(4)
    D, H, N = 16, 6, 50
    W, pi, sigma = rng.normal(size=(D, H)), 0.3, 2.0
    Y = (rng.uniform(size=(N, H)) < pi) @ W.T + sigma * rng.normal(size=(N, D))
    mu = rng.normal(size=D)
    refs = {"bsc": RV.enum_linear(Y, W, sigma, [0., 1.], np.log([1 - pi, pi])),
            "bsc_mu": RV.enum_linear(Y + mu, W, sigma, [0., 1.], np.log([1 - pi, pi]), mu=mu),
            "tsc": RV.enum_linear(Y, W[:, :5], sigma, [-1., 0., 1.], np.log([pi / 2, 1 - pi, pi / 2])),
            "dsc": RV.enum_linear(Y, W[:, :4], sigma, [0., 1., 2., 3.], np.log([0.6, 0.2, 0.1, 0.1])),
            "mca": RV.enum_mca(np.abs(Y), np.abs(W) + 0.1, 21.0, False, 0.25, 0.7),
            "mmca": RV.enum_mca(Y, np.where(np.abs(W) < 0.05, 0.05, W), 6.0, True, 0.25, 0.7)}
    Q = rng.normal(size=(H, H)) * 0.2
    g = {"W": W, "pi": rng.uniform(0.15, 0.45, size=H), "mu": rng.normal(size=H),
         "psi_sq": np.diag(rng.uniform(0.5, 1.5, size=H)) + Q @ Q.T, "sigma_sq": rng.uniform(0.3, 1.2, size=D)}
    refs["gsc"] = RV.enum_gsc(g, Y)
    pies = np.full(H, 1.0 / H)
    refs["mog"] = RV.mog(Y, W, pies, rng.uniform(0.5, 2.0, size=(H, D)))
    refs["mop"] = RV.mop(rng.poisson(3.0, size=(N, D)).astype(np.float64), rng.uniform(0.5, 6.0, size=(D, H)), pies)
    for name, ref in refs.items():
        assert ref.V.shape == (N, D) and (ref.V >= 0).all(), name
        assert _close(ref), name
    # the mean is recon_reference's
    assert R.row_rel_err(refs["bsc"].yhat, R.enum_linear(Y, W, sigma, [0., 1.], np.log([1 - pi, pi]))) < 1e-13
    assert R.row_rel_err(refs["gsc"].yhat, R.enum_gsc(g, Y)) < 1e-13
    # mu shifts the mean and leaves the variance alone
    assert np.abs(refs["bsc_mu"].V - refs["bsc"].V).max() < 1e-12


def test_moments_from_log_joints_give_the_state_sum():
    """m2 / p + finish (what the kernels form) against the sum over the states (what the tests compare with), on BSC's layout
    and on a ternary table with a repeated candidate."""
    rng = np.random.RandomState(5)
    D, H, Hp, N = 7, 9, 4, 30
    W, mu = rng.normal(size=(D, H)), rng.normal(size=D)
    SM = np.array([s for s in np.ndindex(*(2,) * Hp) if sum(s) >= 2], dtype=np.float64)
    cand = np.array([rng.choice(H, size=Hp, replace=False) for _ in range(N)])
    lp = rng.normal(size=(N, 1 + H + len(SM))) * 3
    ref = RV.linear_from_lpj(lp, 1.0, cand, W, (1.0,), 1, 1 + H, SM, mu=mu)
    m2, p = RV.moments2_from_lpj(lp, 1.0, cand, H, (1.0,), 1, 1 + H, SM)
    assert p.shape == (N, 6)
    assert RV.row_err(RV.finish(m2, p, cand, W, ref.yhat, mu), ref) < 1e-13
    T = np.array(list(np.ndindex(3, 3, 3)), dtype=np.float64) - 1.0
    cand = np.array([rng.choice(H, size=3, replace=False) for _ in range(N)])
    cand[::3, 2] = cand[::3, 0]                                              # a repeated candidate: pseudo-states
    lp = rng.normal(size=(N, len(T))) * 3
    ref = RV.linear_from_lpj(lp, 1.0, cand, W, (), 0, 0, T)
    m2, p = RV.moments2_from_lpj(lp, 1.0, cand, H, (), 0, 0, T)
    assert RV.row_err(RV.finish(m2, p, cand, W, ref.yhat), ref) < 1e-13
    assert R.row_rel_err(ref.yhat, R.linear_from_lpj(lp, 1.0, cand, W, (), 0, 0, T)) < 1e-13


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_calibration_identity_on_the_reference(seed):
    """Data drawn from the model, exact posterior: E[(yhat - ybar)^2] = E[V], so the ratio of the sums is 1 up to sampling
    (NumPy enumeration gives 0.986 - 1.018 over seeds 0-9 at these settings).  A condition on the reference, not a measurement."""
    rng = np.random.RandomState(seed)
    D, H, N, pi, sigma = 16, 6, 4000, 0.3, 2.0
    W = rng.normal(size=(D, H))
    clean = (rng.uniform(size=(N, H)) < pi) @ W.T
    Y = clean + sigma * rng.normal(size=(N, D))
    ref = RV.enum_linear(Y, W, sigma, [0., 1.], np.log([1 - pi, pi]))
    ratio = RV.calibration(ref.yhat, ref.V, clean)
    print("calibration seed %d: sum (yhat - clean)^2 / sum V = %.4f" % (seed, ratio))
    assert 0.95 <= ratio <= 1.05
