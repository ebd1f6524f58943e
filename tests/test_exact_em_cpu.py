"""Exact EM for BSC, what needs no device: the NumPy enumeration of tests/exact_em_reference.py pinned against the
oracle at H' = gamma = H and against the closed form for W = c I, the argument checks of pm_moments_exact_* and of the plan
query, the version bump, and every refusal of ``exact_step`` / ``model.exact = True``."""
import ctypes

import numpy as np
import pytest

import exact_em_reference as X
from oracle import bsc_oracle as O

PM_EINVAL, PM_ERANGE = -1, -2


# ---------------------------------------------------------------------------------------------------------- the reference
@pytest.mark.parametrize("H", [3, 6])
@pytest.mark.parametrize("T,prior", [(1.0, False), (1.7, True)])
def test_reference_against_oracle(H, T, prior):
    """oracle/bsc_oracle.py at H' = gamma = H scores every state: its step is the exact one."""
    D, N = 10, 60
    rng = np.random.RandomState(10 * H + int(T))
    params, Y = X.problem(rng, D, H, N)
    an = O.Anneal(T=T, anneal_prior=prior)
    ref, rlog = O.em_step(an, O.make_model(D, H, H, H), dict(params), Y, stats_fn=O.m_step_stats_vec, vec=True)
    new, log = X.step(X.Anneal(T=T, anneal_prior=prior), params, Y)
    assert log["cond"] < 1e6
    np.testing.assert_allclose(new["W"], ref["W"], rtol=1e-9, atol=1e-9 * np.abs(ref["W"]).max())
    np.testing.assert_allclose(new["pi"], ref["pi"], rtol=1e-11)
    np.testing.assert_allclose(new["sigma"], ref["sigma"], rtol=1e-11)
    np.testing.assert_allclose(log["L"], rlog["L"], rtol=1e-11)
    assert log["N_use"] == rlog["N_use"] == N


def test_moments_against_step_totals():
    """The per-row moments add up to the statistics of the step, and Fs is sum v + ecoef sum |x|^2 with the log-odds table."""
    D, H, N = 7, 5, 20
    rng = np.random.RandomState(4)
    params, Y = X.problem(rng, D, H, N, mu=True)
    T = 1.3
    _, log = X.step(X.Anneal(T=T, anneal_prior=True), params, Y)
    beta = 1 / T
    odds = beta * np.log(params["pi"] / (1 - params["pi"]))
    E, C, v = X.moments(Y, params["W"], params["sigma"] / np.sqrt(beta), [0., 1.], np.tile([0., odds], (H, 1)), params["mu"])
    st = log["stats"]
    iu = X.pair_index(H)
    np.testing.assert_allclose(E.sum(0), st["mus"], rtol=1e-12)
    np.testing.assert_allclose(C.sum(0), st["Wq"][iu], rtol=1e-12)
    x2 = ((Y - params["mu"]) ** 2).sum()
    np.testing.assert_allclose(v.sum() - 0.5 * beta / params["sigma"] ** 2 * x2, st["Fs"], rtol=1e-12)
    Wq = np.zeros((H, H))
    Wq[iu] = C.sum(0)
    Wq = Wq + Wq.T - np.diag(np.diag(Wq))
    W = params["W"]
    energy = x2 - 2 * (W.T * (E.T @ (Y - params["mu"]))).sum() + ((W.T @ W) * Wq).sum()
    np.testing.assert_allclose(energy, st["energy"], rtol=1e-10)


def closed_form(Y, c, pi, sigma):
    """W = c I: the latents are independent given y; p_h = sigmoid(logit pi + (c y_h - c^2 / 2) / sigma^2)."""
    H = Y.shape[1]
    a = np.log(pi / (1 - pi)) + (c * Y - 0.5 * c * c) / sigma ** 2
    p = 1.0 / (1.0 + np.exp(-a))
    iu = np.triu_indices(H)
    C = p[:, iu[0]] * p[:, iu[1]]
    C[:, iu[0] == iu[1]] = p
    return p, C


def test_reference_closed_form():
    H, c, pi, sigma = 6, 1.4, 0.3, 0.8
    rng = np.random.RandomState(1)
    Y = rng.normal(size=(5, H)) + c * (rng.random_sample((5, H)) < pi)
    E, C, v = X.moments(Y, c * np.eye(H), sigma, [0., 1.], np.tile(np.log([1 - pi, pi]), (H, 1)))
    p, Cc = closed_form(Y, c, pi, sigma)
    np.testing.assert_allclose(E, p, rtol=1e-12)
    np.testing.assert_allclose(C, Cc, rtol=1e-12)


# ---------------------------------------------------------------------------------------------------------- the C ABI
def _lib():
    from prosper_amd import _lib
    return _lib


def test_version():
    L = _lib()
    assert L.MIN_VERSION >= 1034 and L.load().pm_version() >= 1034 and L.load(True).pm_version() >= 1034
    for name in ("pm_moments_exact_work_len", "pm_moments_exact_plan", "pm_moments_exact_lin_f64"):
        assert name in L.SIGNATURES


def _plan(N, D, K, H):
    out = (ctypes.c_int64 * 12)()
    rc = _lib().load().pm_moments_exact_plan(N, D, K, H, out)
    return rc, list(out)


@pytest.mark.parametrize("det", [False, True])
def test_plan_cells(det):
    """The launch decisions per test case of tests/test_exact_em_abi_gpu.py, and that they never depend on N."""
    rc, p = _plan(5, 8, 2, 6)
    assert rc == 0 and p[:9] == [256, 1, 6, 64, 1, 1, 0, 21, 1]
    rc, p = _plan(3, 8, 2, 1)
    assert rc == 0 and p[2:9] == [1, 2, 1, 1, 0, 1, 1]
    rc, p = _plan(3, 8, 2, 11)
    assert rc == 0 and p[2:9] == [10, 1024, 2, 1, 1, 55, 1]
    rc, p = _plan(67, 8, 2, 13)
    assert rc == 0 and p[2:9] == [10, 1024, 8, 4, 3, 55, 1]
    assert p[9] == 67 * 14 and p[10] == 13 * 67 * 4 and p[11] == 55 * 67 * 1
    rc, p = _plan(3, 8, 2, 15)
    assert rc == 0 and p[2:9] == [10, 1024, 32, 16, 5, 55, 2]
    rc, p = _plan(9, 8, 3, 8)
    assert rc == 0 and p[2:9] == [6, 729, 9, 4, 2, 21, 1]
    rc, p = _plan(4, 8, 3, 10)
    assert rc == 0 and p[2:9] == [6, 729, 81, 40, 4, 21, 5]
    rc, p = _plan(3, 24, 2, 24)
    assert rc == 0 and p[2:9] == [10, 1024, 1 << 14, 256, 14, 55, 256]
    rc, p = _plan(300, 8, 2, 6)
    assert rc == 0 and p[:2] == [256, 2]
    for N in (0, 1, 255, 256, 257, 10 ** 6):
        assert _plan(N, 8, 2, 13)[1][2:9] == [10, 1024, 8, 4, 3, 55, 1]
        assert _plan(N, 8, 2, 20)[1][2:9] == [10, 1024, 1024, 256, 10, 55, 64]
    # the recon plan's split is the same one: E comes from the same sweep
    out = (ctypes.c_int64 * 10)()
    assert _lib().load(det).pm_recon_exact_plan(0, 67, 8, 2, 13, out) == 0 and list(out)[2:6] == [10, 1024, 8, 4]


def test_plan_and_work_len_checks():
    lib = _lib().load()
    assert lib.pm_moments_exact_plan(1, 8, 2, 6, None) == PM_EINVAL
    assert _plan(-1, 8, 2, 6)[0] == PM_EINVAL and _plan(1, 0, 2, 6)[0] == PM_EINVAL and _plan(1, 8, 2, 0)[0] == PM_EINVAL
    assert _plan(1, 8, 1, 6)[0] == PM_EINVAL and _plan(1, 8, 9, 6)[0] == PM_EINVAL
    assert _plan(1, 8, 2, 33)[0] == PM_ERANGE and _plan(1, 8, 3, 21)[0] == PM_ERANGE and _plan(1, 8, 2, 32)[0] == 0
    assert lib.pm_moments_exact_work_len(-1, 6) == -1 and lib.pm_moments_exact_work_len(1, 0) == -1
    assert lib.pm_moments_exact_work_len(0, 6) == 1
    # bounded in N, and enough for the plan's layout
    assert lib.pm_moments_exact_work_len(10 ** 9, 32) == lib.pm_moments_exact_work_len(256, 32)
    for (N, K, H) in ((67, 2, 13), (300, 2, 6), (3, 2, 24), (1000, 2, 32), (9, 3, 8), (4, 3, 10), (5, 2, 1), (300, 8, 10)):
        _, p = _plan(N, 8, K, H)
        assert lib.pm_moments_exact_work_len(N, H) >= p[9] + max(p[10], p[11])


@pytest.mark.parametrize("det", [False, True])
def test_entry_argument_checks(det):
    """Arguments are checked before a device is touched: every call here returns without one."""
    lib = _lib().load(det)
    buf = (ctypes.c_double * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(Y=p, ldy=8, P=p, G=p, logp=p, values=p, K=2, N=1, D=8, H=6, E=p, lde=6, C=p, ldc=21, v=p, work=p):
        return lib.pm_moments_exact_lin_f64(Y, ldy, None, P, G, logp, values, K, N, D, H, E, lde, C, ldc, v, work, None)

    assert call(N=0, Y=None, E=None, C=None, v=None) == 0          # no rows: nothing launched
    for bad in (dict(N=-1), dict(D=0), dict(H=0), dict(K=1), dict(K=9), dict(ldy=7), dict(lde=5), dict(ldc=20), dict(P=None),
                dict(G=None), dict(logp=None), dict(values=None), dict(work=None), dict(Y=None), dict(E=None), dict(C=None),
                dict(v=None)):
        assert call(**bad) == PM_EINVAL, bad
    assert call(N=0, H=33, lde=33, ldc=33 * 17) == PM_ERANGE
    assert call(N=0, K=3, H=21, lde=21, ldc=21 * 11) == PM_ERANGE
    assert call(N=0, H=32, lde=32, ldc=32 * 33 // 2) == 0


# ---------------------------------------------------------------------------------------------------------- refusals
def _model(name, D=8, H=4):
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    from prosper_amd.em.camodels.mmca_et import MMCA_ET
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    from prosper_amd.em.camodels.tsc_et import TSC_ET
    from prosper_amd.em.camodels.gsc_et import GSC
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.em.mixturemodels.MoP import MoP
    if name in ("MoG", "MoP"):
        return {"MoG": MoG, "MoP": MoP}[name](D, H)
    cls = {"BSC_ET": BSC_ET, "MCA_ET": MCA_ET, "MMCA_ET": MMCA_ET, "DSC_ET": DSC_ET, "TSC_ET": TSC_ET, "GSC": GSC}[name]
    return cls(D, H, 3, 2)


OTHERS = ["MCA_ET", "MMCA_ET", "DSC_ET", "TSC_ET", "GSC", "MoG", "MoP"]


def test_attribute_defaults_to_false():
    for name in ["BSC_ET"] + OTHERS:
        m = _model(name)
        assert m.exact is False and "exact" not in m.__dict__


@pytest.mark.parametrize("name", OTHERS)
def test_other_models_refuse(name):
    m = _model(name)
    data = {"y": np.zeros((3, 8))}
    with pytest.raises(NotImplementedError, match=type(m).__name__):
        m.exact_step(X.Anneal(T=1.0), {}, data)
    m.exact = True
    with pytest.raises(NotImplementedError, match=type(m).__name__):
        m.step(X.Anneal(T=1.0), {}, data)


def _bsc_args(D=8, H=4):
    rng = np.random.RandomState(0)
    return {"W": rng.normal(size=(D, H)), "pi": 0.3, "sigma": 1.0}, rng.normal(size=(5, D))


@pytest.mark.parametrize("via_step", [False, True])
@pytest.mark.parametrize("key", ["mask", "weight"])
def test_bsc_refuses_mask_and_weight(key, via_step):
    m = _model("BSC_ET")
    params, Y = _bsc_args()
    data = {"y": Y, key: np.ones_like(Y)}
    if via_step:
        m.exact = True
    with pytest.raises(NotImplementedError, match="exact"):
        (m.step if via_step else m.exact_step)(X.Anneal(T=1.0), params, data)


def test_bsc_refuses_data_noise():
    m = _model("BSC_ET")
    params, Y = _bsc_args()
    with pytest.raises(NotImplementedError, match="data_noise"):
        m.exact_step(X.Anneal(T=1.0, data_noise=0.1), params, {"y": Y})


def test_bsc_refuses_H_33_before_upload():
    """PM_ERANGE from the entry called with no rows -> HipError, with no device on the machine."""
    from prosper_amd._lib import HipError
    m = _model("BSC_ET", D=40, H=33)
    params, Y = _bsc_args(40, 33)
    with pytest.raises(HipError, match="range"):
        m.exact_step(X.Anneal(T=1.0), params, {"y": Y})
    assert getattr(m, "_xe", None) is None and not m._data
