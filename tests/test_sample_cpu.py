"""sample_posterior() without a GPU: tests/sample_reference.py pinned against tests/recon_reference.py -- the
per-state means are the ones reconstruct() averages, stratified uniforms reproduce its estimate within the derived bound for
all eight models, GSC's draws of z have covariance Lambda_s^-1 --, the method and the new C-ABI entries exist in the
signatures, the header, the binding and both libraries, and every refusal comes before anything touches a device."""
import ctypes as C
import inspect
import itertools
import os
import re

import numpy as np
import pytest

import recon_reference as R
import sample_reference as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pm_sample_states_f64", "pm_sample_active_f64", "pm_sample_gsc_f64", "pm_sample_decode_lin_f64",
       "pm_sample_decode_mca_f64")
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


# ------------------------------------------------------------------------------------------------ synthetic E-step outputs
def _case(name, rng, N=5, D=7, H=6, Hp=4, g=2):
    """A truncated posterior made up on the host: random log-joints in the model's column layout, random distinct
    candidates.  Returns a dict with the layout, the reference's posterior mean ``yhat`` (tests/recon_reference.py) and
    ``draw(U, E)`` -> Ys (M, N, D) of tests/sample_reference.py."""
    from prosper_amd.em.camodels import generate_state_matrix
    SM = generate_state_matrix(Hp, g)[2].astype(np.float64)
    cand = np.array([np.sort(rng.permutation(H)[:Hp]) for _ in range(N)])
    W = rng.normal(size=(D, H))
    c = {"name": name, "cand": cand, "H": H, "D": D, "kw": {}}
    if name in ("bsc", "dsc", "tsc"):
        mu = rng.normal(size=D) if name == "bsc" else None
        if name == "bsc":
            blocks, soff, moff, table = (1.0,), 1, 1 + H, SM
        elif name == "dsc":
            blocks, soff, moff = (-1.0, 2.0, 3.0), 1, 1 + 3 * H
            table = SM * rng.choice([-1.0, 2.0, 3.0], size=SM.shape)
        else:
            blocks, soff, moff = (), 0, 0
            table = np.array(list(itertools.product([-1., 0., 1.], repeat=Hp)))
            cand[0, 1] = cand[0, 0]                      # a latent held by two positions
        K = moff + len(table)
        lp = rng.normal(size=(N, K)) * 2
        A = int((table != 0).sum(axis=1).max())
        c.update(K=K, lp=lp, yhat=R.linear_from_lpj(lp, 1.0, cand, W, blocks, soff, moff, table, mu=mu),
                 means=lambda n: SR.state_means_linear(n, cand, W, H, K, blocks, soff, moff, table, mu))

        def draw(U, E=None):
            ai, av = SR.active_list(SR.draw_states(lp, U), cand, H, blocks, soff, moff, table, A)
            return SR.decode_linear(ai, av, W, mu)
    elif name in ("mca", "mmca"):
        signed = name == "mmca"
        W = rng.uniform(-2, 3, size=(D, H)) if signed else rng.uniform(0.1, 3, size=(D, H))
        rho = 6.0 if signed else 21.0
        K = 1 + H + len(SM)
        lp = rng.normal(size=(N, K)) * 2
        c.update(K=K, lp=lp, yhat=R.mca_from_lpj(lp, cand, SM, W, rho, signed),
                 means=lambda n: SR.decode_mca(np.arange(K, dtype=np.int32)[None, :], cand[n:n + 1], SM, W, rho, signed)[:, 0])

        def draw(U, E=None):
            return SR.decode_mca(SR.draw_states(lp, U), cand, SM, W, rho, signed)
    elif name in ("mog", "mop"):
        K = H
        lp = rng.normal(size=(N, K)) * 2
        off = rng.normal(size=K)
        a = -0.5 if name == "mog" else 1.0                   # (MoG full: a = -1/2 on the Mahalanobis terms, offsets beside)
        c.update(K=K, lp=lp, yhat=R.softmax_rows(a * lp + off[None, :]) @ W.T, means=lambda n: W.T.copy(),
                 kw=dict(a=a, off=off))

        def draw(U, E=None):
            idx = SR.draw_states(lp, U, a=a, off=off)
            ai, av = SR.active_list(idx, None, H, (1.0,), 0, 0, None, 1)
            return SR.decode_linear(ai, av, W)
    else:
        Q = rng.normal(size=(H, H)) * 0.2
        p = {"W": W, "pi": rng.uniform(0.15, 0.45, size=H), "mu": rng.normal(size=H),
             "psi_sq": np.diag(rng.uniform(0.5, 1.5, size=H)) + Q @ Q.T, "sigma_sq": np.float64(0.6)}
        Y = rng.normal(size=(N, D))
        K = 1 + H + len(SM)
        lp = rng.normal(size=(N, K)) * 2
        kw = dict(SR.GSC_WEIGHTS, lse=np.zeros(N))

        def means(n):
            out = np.zeros((K, D))
            for k in range(1, K):
                act = [k - 1] if k <= H else list(cand[n, np.nonzero(SM[k - 1 - H])[0]])
                out[k] = W[:, act] @ SR.gsc_posterior(p, Y[n], act)[0]
            return out
        c.update(K=K, lp=lp, yhat=R.gsc_from_lpj(p, Y, lp, cand, SM), means=means, kw=kw, p=p, Y=Y, SM=SM)

        def draw(U, E=None):
            E = np.zeros(U.shape + (g,)) if E is None else E
            ai, av = SR.gsc_active_list(SR.draw_states(lp, U, **kw), cand, SM, p, Y, E, g)
            return SR.decode_linear(ai, av, W)
    c["draw"] = draw
    return c


EIGHT = ["bsc", "dsc", "tsc", "mca", "mmca", "gsc", "mog", "mop"]


@pytest.mark.parametrize("name", EIGHT)
def test_per_state_means_are_the_ones_reconstruct_averages(name):
    """sum_k q_k ybar(k) with the reference's per-state means equals recon_reference's posterior mean."""
    c = _case(name, np.random.RandomState(3))
    w = SR.weights(c["lp"], **c["kw"])
    q = w / w.sum(axis=1, keepdims=True)
    got = np.stack([q[n] @ c["means"](n) for n in range(len(q))])
    np.testing.assert_allclose(got, c["yhat"], rtol=0, atol=1e-12 * np.abs(c["yhat"]).max())


@pytest.mark.parametrize("name", EIGHT)
def test_stratified_uniforms_reproduce_the_posterior_mean(name):
    """u_m = (m + 1/2) / M (GSC: eps = 0): state k is drawn count_k times with |count_k - M q_k| < 1 -- the stratified points
    that fall into an interval of length q_k number floor(M q_k) or ceil(M q_k) --, so |mean_m Ys - yhat|_d <= sum_k |count_k /
    M - q_k| |ybar_d(k)| < (K / M) max_k |ybar_d(k)|."""
    c = _case(name, np.random.RandomState(4))
    M = 4000
    N, K = c["lp"].shape
    Ys = c["draw"](np.tile(SR.stratified(M), (N, 1)))
    assert Ys.shape == (M, N, c["D"])
    for n in range(N):
        bound = (K / M) * np.abs(c["means"](n)).max(axis=0)
        err = np.abs(Ys[:, n].mean(axis=0) - c["yhat"][n])
        assert (err <= bound).all(), (name, n, err.max(), bound.min())


def test_draw_rule_edges():
    """u = 0 / the largest double below 1 hit the first / last column of positive weight, a column of weight 0 is skipped,
    a u outside [0, 1) or NaN is clamped, a NaN row gives -1 and disturbs no other row."""
    with np.errstate(divide="ignore"):
        lp = np.log(np.array([[0., 2., 0., 1., 1., 0.], [1., 1., 1., 1., 1., 1.], [1., np.nan, 1., 1., 1., 1.]]))
    U = np.array([[0.0, SR.U_MAX, 0.5, -3.0, 7.0, np.nan]] * 3)
    idx = SR.draw_states(lp, U)
    assert idx[0].tolist() == [1, 4, 3, 1, 4, 1]
    assert idx[1].tolist() == [0, 5, 3, 0, 5, 0]
    assert (idx[2] == -1).all()
    mids = (np.arange(6) + 0.5) / 6
    assert SR.draw_states(lp[1:2], mids[None, :])[0].tolist() == list(range(6))


def test_uniforms_on_a_cdf_edge_are_moved_to_the_middle_of_an_interval():
    """What the device tests do before they compare indices: a u within 1e-9 of an edge goes to the middle of the interval of
    the column the reference draws (the next wide one if that is a sliver); the others stay, none is dropped."""
    lp = np.log(np.array([[1., 2., 1., 4.]]))
    c = SR.cdfs(lp)
    U = np.array([[0.125, 0.125 + 1e-12, 0.3, 0.5 - 1e-11, 0.0, 0.9]])
    V, moved = SR.nudge(U, c)
    assert moved == 4 and V.shape == U.shape
    np.testing.assert_allclose(V[0], [0.25, 0.25, 0.3, 0.4375, 0.0625, 0.9], rtol=1e-12)
    assert SR.draw_states(lp, V)[0].tolist() == [1, 1, 1, 2, 0, 3]
    # the move changes nothing for a CDF summed in another order: the draws are those of the perturbed edges too
    assert SR.draw_states(lp + 1e-13 * np.array([[1., -1., 1., -1.]]), V)[0].tolist() == [1, 1, 1, 2, 0, 3]


def test_gsc_draws_of_a_fixed_state_have_covariance_lambda_inverse():
    """With eps the 2 gamma signed vectors +-sqrt(gamma) e_i: mean_m (z_m - kappa)(z_m - kappa)^T = L L^T = Lambda_s^-1."""
    c = _case("gsc", np.random.RandomState(5), H=8, Hp=5, g=4)
    p, Y = c["p"], c["Y"]
    for act in ([2], [1, 4], [0, 3, 6], [1, 2, 5, 7]):
        g = len(act)
        eps = np.sqrt(g) * np.concatenate([np.eye(g), -np.eye(g)])
        kappa, cov = SR.gsc_posterior(p, Y[0], act)
        Z = np.stack([SR.gsc_draw(p, Y[0], act, e) for e in eps])
        np.testing.assert_allclose(Z.mean(axis=0), kappa, rtol=0, atol=1e-13 * np.abs(kappa).max())
        got = (Z - kappa).T @ (Z - kappa) / len(eps)
        assert np.abs(got - cov).max() <= 1e-11 * np.abs(cov).max()
        want = np.linalg.inv(p["W"][:, act].T @ p["W"][:, act] / 0.6 + np.linalg.inv(p["psi_sq"][np.ix_(act, act)]))
        assert np.abs(cov - want).max() <= 1e-11 * np.abs(want).max()


# ----------------------------------------------------------------------------------------------- the surface is there
def test_every_model_has_the_method_and_no_exact_keyword():
    ca, mix = _models()
    for cls in ca + mix:
        par = inspect.signature(cls.sample_posterior).parameters
        assert list(par) == ["self", "model_params", "my_data", "n_samples", "seed", "latents", "device", "uniforms",
                             "normals"], cls.__name__
        assert par["n_samples"].default == 1 and par["seed"].default is None and par["latents"].default is False
        assert "exact" not in par
        doc = cls.sample_posterior.__doc__
        assert "depend on (my_N, n_samples)" in doc and "noise is not added" in doc.replace("NOT", "not"), cls.__name__


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
    assert _lib.load().pm_version() >= 1027 and _lib.MIN_VERSION >= 1027
    assert _lib.load(True).pm_version() >= _lib.MIN_VERSION
    assert _lib.load().pm_sample_states_max_cols() >= 1 + 1024 + 2516       # H = 1024 with H' = 16, gamma = 3 and far beyond


# ------------------------------------------------------------------------------------------- refusals before any launch
def test_argument_refusals_come_before_any_device_call():
    """No device on this machine: a refusal that came after a look at the device would raise HipError."""
    ca, mix = _models()
    y = np.zeros((3, 4))
    for model in [cls(4, 4, 2, 2) for cls in ca] + [cls(4, 4) for cls in mix]:
        name = type(model).__name__
        for bad in (0, -1, 1.5):
            with pytest.raises(ValueError, match="n_samples"):
                model.sample_posterior({}, {'y': y}, n_samples=bad)
        for shape in ((3,), (3, 3), (2, 2), (3, 2, 1)):
            with pytest.raises(ValueError, match="uniforms has shape"):
                model.sample_posterior({}, {'y': y}, n_samples=2, uniforms=np.zeros(shape))
        for v in (1.0, -1e-300, np.nan, np.inf):
            u = np.full((3, 2), 0.25)
            u[1, 1] = v
            with pytest.raises(ValueError, match=r"uniforms must lie in \[0, 1\)"):
                model.sample_posterior({}, {'y': y}, n_samples=2, uniforms=u)
        with pytest.raises(TypeError):
            model.sample_posterior({}, {'y': y}, exact=True)
        if name == "GSC":
            for shape in ((3, 2), (3, 2, 3), (2, 2, 2)):
                with pytest.raises(ValueError, match="normals has shape"):
                    model.sample_posterior({}, {'y': y}, n_samples=2, normals=np.zeros(shape))


def test_a_mask_on_the_other_models_keeps_its_refusal():
    ca, mix = _models()
    y, m = np.zeros((3, 4)), np.ones((3, 4), dtype=bool)
    for model in [cls(4, 4, 2, 2) for cls in ca[3:]] + [cls(4, 4) for cls in mix]:
        with pytest.raises(NotImplementedError, match=type(model).__name__ + r".*mask"):
            model.sample_posterior({}, {'y': y, 'mask': m})
    for cls in ca[:3]:
        with pytest.raises(ValueError, match="mask"):
            cls(4, 4, 2, 2).sample_posterior({}, {'y': y, 'mask': m[:2]})


def test_one_past_each_limit_is_refused_by_name():
    from prosper_amd import _lib
    ca, _ = _models()
    for cls in ca[:4]:             # (TSC's constructor enumerates 3^17 states: minutes; the refusal is the same line)
        model = cls(4, 40, 17, 2)
        with pytest.raises(_lib.HipError, match="sample_posterior holds H' <= 16"):
            model.sample_posterior({}, {'y': np.zeros((3, 4))})
    for cls in ca[1:3]:
        with pytest.raises(_lib.HipError, match="sample_posterior holds D <= 1024"):
            cls(1025, 8, 4, 2).sample_posterior({}, {'y': np.zeros((3, 1025))})


def test_no_rows_give_empty_arrays():
    ca, mix = _models()
    for model in [cls(4, 4, 2, 2) for cls in ca] + [cls(4, 4) for cls in mix]:
        out = model.sample_posterior({}, {'y': np.zeros((0, 4))}, n_samples=3)
        assert out.shape == (3, 0, 4) and out.dtype == np.float64
        Ys, S = model.sample_posterior({}, {'y': np.zeros((0, 4))}, n_samples=2, latents=True)
        assert Ys.shape == (2, 0, 4) and S.shape == (2, 0, 4)


# ---------------------------------------------------------------------------------------------------- argument checks
@pytest.mark.parametrize("det", [False, True])
def test_entries_reject_bad_arguments_without_a_device(det):
    """Every pointer below is host memory (or NULL): a launch would fault, a correct entry returns before one."""
    from prosper_amd import _lib
    lib = _lib.load(det)
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    one = (C.c_double * 8)(1.0)

    def states(lp=p, ld=10, lse=None, a=1.0, off=None, floor=0.0, null=-1, U=p, ldu=3, N=4, K=9, M=3, idx=p):
        return lib.pm_sample_states_f64(lp, ld, lse, a, off, floor, null, U, ldu, N, K, M, idx, None)
    for k in ("lp", "U", "idx"):
        assert states(**{k: None}) == PM_EINVAL, k
        assert states(N=0, **{k: None}) == PM_EINVAL, k
    assert states(N=-1) == PM_EINVAL and states(K=0) == PM_EINVAL and states(M=0) == PM_EINVAL and states(ld=8) == PM_EINVAL
    assert states(ldu=2) == PM_EINVAL and states(floor=-1.0) == PM_EINVAL and states(floor=float("nan")) == PM_EINVAL
    assert states(null=9) == PM_EINVAL and states(null=-2) == PM_EINVAL
    big = int(lib.pm_sample_states_max_cols()) + 1
    assert states(K=big, ld=big) == PM_ERANGE
    assert states(N=0) == 0 and states(N=0, lse=p, a=0.5, floor=1e-300, null=0) == 0

    def active(idx=p, cand=p, vals=p, bv=one, N=4, M=3, H=4, Hp=3, K=9, soff=1, nblk=1, moff=5, S=4, A=2, ai=p, av=p):
        return lib.pm_sample_active_f64(idx, cand, vals, bv, N, M, H, Hp, K, soff, nblk, moff, S, A, ai, av, None)
    for k in ("idx", "cand", "vals", "bv", "ai", "av"):
        assert active(**{k: None}) == PM_EINVAL, k
        assert active(N=0, **{k: None}) == PM_EINVAL, k
    assert active(N=-1) == PM_EINVAL and active(M=0) == PM_EINVAL and active(H=0) == PM_EINVAL and active(A=0) == PM_EINVAL
    assert active(moff=6) == PM_EINVAL and active(nblk=3) == PM_EINVAL and active(Hp=0) == PM_EINVAL and active(S=-1) == PM_EINVAL
    assert active(Hp=17) == PM_ERANGE and active(A=17) == PM_ERANGE and active(nblk=9, K=200) == PM_ERANGE
    assert active(N=0) == 0 and active(N=0, S=0, moff=0, Hp=0, cand=None, vals=None) == 0

    def gsc(idx=p, cand=p, masks=p, sc=p, lds=4, G=p, psi=p, tab=p, s2=0.6, E=p, lde=2, N=4, M=3, H=4, Hp=3, S=4, gamma=2, A=2,
            ai=p, av=p):
        return lib.pm_sample_gsc_f64(idx, cand, masks, sc, lds, G, psi, tab, s2, E, lde, N, M, H, Hp, S, gamma, A, ai, av, None)
    for k in ("idx", "cand", "masks", "sc", "G", "psi", "tab", "E", "ai", "av"):
        assert gsc(**{k: None}) == PM_EINVAL, k
        assert gsc(N=0, **{k: None}) == PM_EINVAL, k
    assert gsc(N=-1) == PM_EINVAL and gsc(M=0) == PM_EINVAL and gsc(H=0) == PM_EINVAL and gsc(Hp=0) == PM_EINVAL
    assert gsc(lds=3) == PM_EINVAL and gsc(lde=1) == PM_EINVAL and gsc(A=1) == PM_EINVAL and gsc(gamma=0) == PM_EINVAL
    assert gsc(s2=0.0) == PM_EINVAL and gsc(s2=float("nan")) == PM_EINVAL
    assert gsc(gamma=9, A=9, lde=9) == PM_ERANGE and gsc(Hp=17) == PM_ERANGE and gsc(A=17) == PM_ERANGE
    assert gsc(N=0) == 0 and gsc(N=0, S=0, cand=None, masks=None, G=None, psi=None) == 0

    def lin(ai=p, av=p, A=2, Wt=p, ldw=10, mu=None, N=4, M=3, H=4, D=10, out=p, ldn=10, ldm=40):
        return lib.pm_sample_decode_lin_f64(ai, av, A, Wt, ldw, mu, N, M, H, D, out, ldn, ldm, None)
    for k in ("ai", "av", "Wt", "out"):
        assert lin(**{k: None}) == PM_EINVAL, k
        assert lin(N=0, **{k: None}) == PM_EINVAL, k
    assert lin(N=-1) == PM_EINVAL and lin(M=0) == PM_EINVAL and lin(H=0) == PM_EINVAL and lin(D=0) == PM_EINVAL
    assert lin(A=0) == PM_EINVAL and lin(ldw=9) == PM_EINVAL and lin(ldn=9) == PM_EINVAL and lin(ldm=9) == PM_EINVAL
    assert lin(A=17) == PM_ERANGE
    assert lin(N=0) == 0 and lin(N=0, mu=p) == 0

    def mca(idx=p, cand=p, masks=p, Wt=p, Wrho=p, inv_rho=1 / 21., N=4, M=3, H=4, D=10, Hp=2, S=1, out=p, ldn=None, ldm=None):
        return lib.pm_sample_decode_mca_f64(idx, cand, masks, Wt, Wrho, inv_rho, 0, N, M, H, D, Hp, S, out,
                                            D if ldn is None else ldn, N * D if ldm is None else ldm, None)
    for k in ("idx", "cand", "masks", "Wt", "Wrho", "out"):
        assert mca(**{k: None}) == PM_EINVAL, k
        assert mca(N=0, ldm=40, **{k: None}) == PM_EINVAL, k
    assert mca(N=-1, ldm=40) == PM_EINVAL and mca(M=0) == PM_EINVAL and mca(Hp=0) == PM_EINVAL and mca(ldn=9) == PM_EINVAL
    assert mca(ldm=9) == PM_EINVAL and mca(inv_rho=0.0) == PM_EINVAL and mca(S=-1) == PM_EINVAL
    assert mca(D=1025) == PM_ERANGE and mca(Hp=17) == PM_ERANGE
    assert mca(N=0, ldm=40) == 0 and mca(N=0, ldm=40, S=0, cand=None, masks=None, Wrho=None) == 0
