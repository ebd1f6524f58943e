"""Every documented limit of the HIP path fails LOUDLY -- `HipError` (PM_ERANGE from the library, or
the host's own range check) -- and never returns a wrong answer or falls back to a CPU path.  The reference itself asserts
only H' <= H and gamma <= H' (camodels/__init__.py:90-91)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


class _An(dict):
    crit_params = []

    def __missing__(self, k):
        return 0.0

    def as_dict(self):
        return dict(self)


def _data(D, H, N, seed=0, positive=False):
    rng = np.random.RandomState(seed)
    W = rng.normal(size=(D, H))
    if positive:
        W = np.abs(W) + 0.1
    y = (rng.random_sample((N, H)) < 2.0 / H) @ W.T + rng.normal(size=(N, D))
    return W, y


def _bsc(D, H, Hp, g):
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    W, y = _data(D, H, 40)
    return BSC_ET(D, H, Hp, g), {"W": W, "pi": 2.0 / H, "sigma": 1.0}, y


def _mca(D, H, Hp, g, cls="MCA_ET"):
    import importlib
    mod = importlib.import_module("prosper_amd.em.camodels." + ("mca_et" if cls == "MCA_ET" else "mmca_et"))
    W, y = _data(D, H, 40, positive=True)
    return getattr(mod, cls)(D, H, Hp, g), {"W": W, "pi": 2.0 / H, "sigma": 1.0}, y


def _dsc(D, H, Hp, g, states):
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    W, y = _data(D, H, 40)
    K = len(states)
    pi = np.full(K, 0.5 / (K - 1))
    pi[list(states).index(0.0)] = 0.5
    return DSC_ET(D, H, Hp, g, states=np.array(states)), {"W": W, "pi": pi, "sigma": 1.0}, y


def _tsc(D, H, Hp, g):
    from prosper_amd.em.camodels.tsc_et import TSC_ET
    W, y = _data(D, H, 40)
    return TSC_ET(D, H, Hp, g), {"W": W, "pi": 2.0 / H, "sigma": 1.0}, y


def _gsc(D, H, Hp, g):
    from prosper_amd.em.camodels.gsc_et import GSC
    W, y = _data(D, H, 40)
    return GSC(D, H, Hp, g, "scalar"), {"W": W, "pi": np.full(H, 2.0 / H), "mu": np.ones(H), "psi_sq": np.eye(H),
                                        "sigma_sq": 1.0}, y


BEYOND = [
    ("BSC H > 1024", lambda: _bsc(16, 1100, 4, 2)),
    ("BSC H' > 16", lambda: _bsc(16, 40, 17, 2)),
    ("MCA H > 512", lambda: _mca(16, 600, 4, 2)),
    ("MCA H' > 16", lambda: _mca(16, 40, 17, 2)),
    ("MCA E-step D > 1024", lambda: _mca(1100, 12, 4, 2)),
    ("MMCA H > 512", lambda: _mca(16, 600, 4, 2, "MMCA_ET")),
    ("DSC more than 8 latent values", lambda: _dsc(16, 12, 3, 2, [-4., -3., -2., -1., 0., 1., 2., 3., 4.])),
    ("DSC H > 512", lambda: _dsc(16, 600, 4, 2, [-1., 0., 1.])),
    ("TSC 2 H > 512", lambda: _tsc(16, 300, 4, 2)),
    ("GSC H > 512", lambda: _gsc(16, 600, 4, 2)),
    ("GSC gamma > 8", lambda: _gsc(16, 12, 10, 9)),
    # the E-step's LDS (8 H + 16 (48 + 4 H'^2) + S / 4 doubles, gsc_kernels.hip gsc_shmem) passes 64 KB: at H' = 8 above H = 408
    ("GSC H' = 8, H = 409", lambda: _gsc(16, 409, 8, 8)),
    ("GSC H' = 8, H = 512", lambda: _gsc(16, 512, 8, 5)),
]


@pytest.mark.parametrize("what,make", BEYOND, ids=[b[0] for b in BEYOND])
def test_beyond_a_documented_limit_raises(what, make):
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU box (MI355X)")
    from prosper_amd import _lib
    with pytest.raises(_lib.HipError):
        model, params, y = make()             # (some limits are checked by the constructor)
        model.step(_An(T=1.0), params, {"y": y})


WITHIN = [
    ("BSC H = 1024 (generic row kernels, blocked inverse)", lambda: _bsc(16, 1024, 4, 2)),
    ("BSC H' = 16", lambda: _bsc(24, 40, 16, 2)),
    ("MCA H' = 16", lambda: _mca(24, 40, 16, 2)),
    ("MCA D = 1024", lambda: _mca(1024, 12, 4, 2)),
    ("DSC 8 latent values", lambda: _dsc(16, 12, 3, 2, [-3., -2., -1., 0., 1., 2., 3., 4.])),
    ("TSC 2 H = 512", lambda: _tsc(16, 256, 4, 2)),
    ("GSC gamma = 8", lambda: _gsc(16, 12, 9, 8)),
    ("GSC H' = 8, H = 408, gamma = 8 (64 KB of LDS)", lambda: _gsc(16, 408, 8, 8)),
]


def _cp(p):
    return {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in p.items()}


def _against_oracle(model, params, y):
    """E-step log-joints on the model's candidates (which must be the oracle's) and one ``step`` of a fresh copy of the model
    against the plain-NumPy oracle; returns the new parameters."""
    kind = type(model).__name__
    D, H, Hp, g = model.D, model.H, model.Hprime, model.gamma
    fresh = {"BSC_ET": lambda: _bsc(D, H, Hp, g)[0], "MCA_ET": lambda: _mca(D, H, Hp, g)[0],
             "DSC_ET": lambda: _dsc(D, H, Hp, g, list(model.states))[0], "TSC_ET": lambda: _tsc(D, H, Hp, g)[0],
             "GSC": lambda: _gsc(D, H, Hp, g)[0]}[kind]
    an = _An(T=1.0)
    if kind == "GSC":
        from oracle import gsc_oracle as G
        om = G.make_model(D, H, Hp, g)
        lpj, cand = model.compute_lpj(an, _cp(params), {"y": y})
        cand = np.asarray(cand).astype(np.int64)
        assert np.array_equal(cand, G.select_hprimes(params, y, Hp))
        np.testing.assert_allclose(np.asarray(lpj), G.compute_lpj(om, params, y, cand), rtol=1e-9, atol=1e-8)
        ref, log = G.em_step(G.Anneal(T=1.0), om, _cp(params), y)
        new = fresh().step(an, _cp(params), {"y": y})
        tol = max(1e-8, 50 * np.linalg.cond(log["suff"]["xpt_szsz"].sum(0)) * np.finfo(float).eps)
        for k in ("W", "pi", "mu", "psi_sq", "sigma_sq"):
            np.testing.assert_allclose(new[k], ref[k], rtol=10 * tol, atol=tol * max(1.0, np.abs(ref[k]).max()), err_msg=k)
        return new
    if kind == "BSC_ET":
        from oracle import bsc_oracle as O
        ref, log = O.em_step(O.Anneal(T=1.0, Ncut_factor=0.0, anneal_prior=False), O.make_model(D, H, Hp, g), _cp(params), y,
                             stats_fn=O.m_step_stats_vec, vec=True)
    elif kind == "MCA_ET":
        from oracle import mca_oracle as O
        params = model.check_params(_cp(params))
        ref, log = O.em_step(O.Anneal(T=1.0, Ncut_factor=0.0), O.make_model(D, H, Hp, g), _cp(params), y, vec=True)
    else:
        import importlib
        O = importlib.import_module("oracle.%s_oracle" % kind[:3].lower())
        om = O.make_model(D, H, Hp, g, np.array(model.states)) if kind == "DSC_ET" else O.make_model(D, H, Hp, g)
        ref, log = O.em_step(O.Anneal(T=1.0, Ncut_factor=0.0, anneal_prior=False), om, _cp(params), y, vec=True)
    data = model.select_Hprimes(_cp(params), {"y": y})
    ss = model.E_step(an, _cp(params), data)
    cand = np.asarray(data["candidates"]).astype(np.int64)
    if kind == "MCA_ET" and not np.array_equal(cand, log["candidates"]):
        # (MCA ranks candidates by distances that tie exactly where a latent's column does not change the datapoint's
        # reconstruction at all -- test_gsc_gamma4_and_mca_hprime10_match_the_oracle: the same SET of scores is required, and the
        # rest is compared on the device's candidates)
        sc = O.select_scores_vec(params["W"], y)
        assert np.array_equal(np.sort(np.take_along_axis(sc, cand, 1), 1), np.sort(np.take_along_axis(sc, log["candidates"], 1), 1))
        om = O.make_model(D, H, Hp, g)
        an_o = O.Anneal(T=1.0, Ncut_factor=0.0)
        lp = O.e_step_vec(an_o, params["W"], params["pi"], params["sigma"], y, cand, om["SM"], om["state_abs"])
        ref, log = O.m_step(an_o, om, params["W"], params["pi"], params["sigma"], y, cand, lp, vec=True)
        log["logpj"] = lp
    else:
        assert np.array_equal(cand, log["candidates"])
    np.testing.assert_allclose(np.asarray(ss["logpj"]), log["logpj"], rtol=1e-10, atol=1e-9)
    new = fresh().step(an, _cp(params), {"y": y})
    np.testing.assert_allclose(new["pi"], ref["pi"], rtol=1e-9)
    np.testing.assert_allclose(new["sigma"], ref["sigma"], rtol=1e-9)
    if kind == "MCA_ET":          # (element-wise W update)
        np.testing.assert_allclose(new["W"], ref["W"], rtol=1e-8, atol=1e-10)
        return new
    # W_new solves Wq X = Wp: the comparison is scaled by the conditioning of Wq; with N < H it is singular, and W_new is
    # defined only up to the SVD cutoff of the reference's lstsq -- then pi, sigma and the log-joints above pin the step
    cond = np.linalg.cond(log["stats"]["Wq"])
    if cond < 1e10:
        tol = max(1e-8, 20 * cond * np.finfo(float).eps)
        np.testing.assert_allclose(new["W"], ref["W"], rtol=10 * tol, atol=tol * np.abs(ref["W"]).max())
    return new


@pytest.mark.parametrize("what,make", WITHIN, ids=[w[0] for w in WITHIN])
def test_at_a_documented_limit_runs(what, make):
    """... and AT the limit a step runs, returns finite parameters and agrees with the oracle: candidates and E-step
    log-joints, then one whole step."""
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU box (MI355X)")
    model, params, y = make()
    new = _against_oracle(model, params, y)
    assert np.isfinite(np.asarray(new["W"])).all()


# ---------------------------------------------------------------------------------------------- off-config shapes
_SWEEP = [(256, 128, 6, 3, 300), (1024, 256, 6, 3, 200), (1024, 256, 10, 4, 120), (784, 400, 8, 3, 120), (1024, 512, 8, 4, 96),
          (4096, 1024, 10, 3, 40)]


@pytest.mark.parametrize("D,H,Hp,gamma,N", _SWEEP)
def test_bsc_off_config_shapes_match_the_oracle(D, H, Hp, gamma, N):
    """The shapes bench.py's `other_shapes` times (the reference accepts any H' <= H, gamma <= H'; BASELINE names one): whichever
    code path the host layer picks for them -- the 4-wavefront one-kernel pass, scores GEMM + 16-lane row kernel (now with up to
    the CU's whole LDS), the generic kernels -- candidates, log-joints and the M-step agree with the oracle."""
    from oracle import bsc_oracle as O
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    rng = np.random.RandomState(D + H + Hp)
    W_gt = rng.normal(size=(D, H))
    y, _ = O.generate_bsc_data(W_gt, 4.0 / H, 1.0, N, rng)
    params = {"W": W_gt + 0.1 * rng.normal(size=(D, H)), "pi": 4.0 / H, "sigma": 1.1}
    an = O.Anneal(T=1.1, Ncut_factor=0.0, anneal_prior=False)
    an.crit_params = []
    ref, log = O.em_step(an, O.make_model(D, H, Hp, gamma), dict(params), y, stats_fn=O.m_step_stats_vec, vec=True)
    m = BSC_ET(D, H, Hp, gamma)
    data = m.select_Hprimes(params, {"y": y})
    ss = m.E_step(_An(T=1.1), params, data)
    cand = np.asarray(data["candidates"]).astype(np.int64)
    same = (cand == log["candidates"]).all(axis=1)
    if not same.all():
        # a near-tie of the ranked scores (the device's come out of a split-K GEMM whose atomics sum in run-to-run order:
        # seen once in a few hundred runs at H = 512); anything else is a defect
        sc = (y @ params["W"]) / np.sqrt((params["W"] ** 2).sum(axis=0))[None, :]
        a, b = (np.sort(np.take_along_axis(sc[~same], c[~same], 1), axis=1) for c in (cand, log["candidates"]))
        np.testing.assert_allclose(a, b, rtol=1e-11, atol=1e-11 * np.abs(sc).max())
        pytest.skip("selection near-tie on this run: the rest of the comparison assumes the oracle's candidates")
    np.testing.assert_allclose(np.asarray(ss["logpj"]), log["logpj"], rtol=1e-10, atol=1e-8)
    new = m.M_step(_An(T=1.1), params, ss, data)
    # (N < H: Wq is rank-deficient and W_new is only defined up to LAPACK's SVD cutoff -- the statistics pin the path)
    np.testing.assert_allclose(new["pi"], ref["pi"], rtol=1e-9)
    np.testing.assert_allclose(new["sigma"], ref["sigma"], rtol=1e-9)
    st, lib = m._ws["stats"].cpu().numpy(), __import__("prosper_amd._lib", fromlist=["load"]).load()
    Wp = st[:lib.pm_bsc_stats_offset_wq(H, D)].reshape(H, D)
    np.testing.assert_allclose(Wp, log["stats"]["Wp"], rtol=1e-9, atol=1e-9 * np.abs(log["stats"]["Wp"]).max())


def test_gsc_gamma4_and_mca_hprime10_match_the_oracle():
    """GSC at config-4 dimensions with gamma = 4 (the g x g systems in registers at one wavefront per SIMD) and MCA at config-5
    dimensions with H' = 10: the other two entries of bench.py's `other_shapes`."""
    from oracle import gsc_oracle as G, mca_oracle as M, bsc_oracle as B
    from prosper_amd.em.camodels.gsc_et import GSC
    from prosper_amd.em.camodels.mca_et import MCA_ET
    D, H = 256, 128
    rng = np.random.RandomState(5)
    gt = {"W": rng.normal(size=(D, H)), "pi": np.full(H, 2.0 / H), "mu": np.full(H, 1.5), "psi_sq": np.eye(H), "sigma_sq": 1.0}
    y, _, _ = G.generate_gsc_data(gt, 700, rng)
    params = {"W": gt["W"] + 0.1 * rng.normal(size=(D, H)), "pi": gt["pi"] * 1.1, "mu": gt["mu"] + 0.1 * rng.normal(size=H),
              "psi_sq": np.diag(rng.uniform(0.7, 1.4, size=H)), "sigma_sq": 1.2}
    cp = lambda q: {k: np.array(v, copy=True) for k, v in q.items()}
    ref, log = G.em_step(G.Anneal(T=1.0), G.make_model(D, H, 6, 4), cp(params), y)
    new = GSC(D, H, 6, 4, "scalar").step(_An(T=1.0), cp(params), {"y": y})
    tol = max(1e-8, 50 * np.linalg.cond(log["suff"]["xpt_szsz"].sum(0)) * np.finfo(float).eps)
    for k in ("W", "pi", "mu", "psi_sq", "sigma_sq"):
        np.testing.assert_allclose(new[k], ref[k], rtol=10 * tol, atol=tol * max(1.0, np.abs(ref[k]).max()), err_msg=k)
    Wm = np.abs(rng.normal(size=(D, H))) * 2 + 0.1
    ym, _ = M.generate_mca_data(Wm, 2.0 / H, 1.0, 300, rng)
    pm = {"W": Wm * rng.uniform(0.9, 1.1, size=Wm.shape), "pi": 2.0 / H, "sigma": 1.0}
    refm, logm = M.em_step(B.Anneal(T=1.0), B.make_model(D, H, 10, 3), dict(pm), ym, vec=True)
    mm = MCA_ET(D, H, 10, 3)
    data = mm.select_Hprimes(mm.check_params(dict(pm)), {"y": ym})
    if np.array_equal(np.asarray(data["candidates"]).astype(np.int64), logm["candidates"]):     # (no tie of zero distances)
        newm = mm.step(_An(T=1.0), dict(pm), {"y": ym})
        np.testing.assert_allclose(newm["W"], refm["W"], rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(newm["pi"], refm["pi"], rtol=1e-9)
        np.testing.assert_allclose(newm["sigma"], refm["sigma"], rtol=1e-9)
    else:
        sc = M.select_scores_vec(M.check_params(dict(pm))["W"], ym)
        got = np.asarray(data["candidates"]).astype(np.int64)
        assert np.array_equal(np.sort(np.take_along_axis(sc, got, 1), 1), np.sort(np.take_along_axis(sc, logm["candidates"], 1), 1))


@pytest.mark.parametrize("model,N", [("bsc", 1), ("bsc", 7), ("mca", 1), ("mca", 9), ("mmca", 5)])
def test_a_truncation_rank_of_zero_keeps_everything_as_upstream(model, N):
    """Round 6 (scratch/fuzz_shapes.py): on a handful of datapoints ``int(N (1 - (1 - A) Ncut_factor))`` is 0, and upstream's
    ``allsort(...)[-0]`` is the SMALLEST evidence -- every datapoint is kept (bsc_et.py:251-253, mca_et.py:255-258).  The host
    layer used to divide by that zero."""
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU box (MI355X)")
    D, H, Hp, gamma = 24, 12, 4, 1         # (pi = 0.4, gamma = 1: A = P(|s| <= 1) = 0.02 -> int(N A) = 0 up to N = 50)
    rng = np.random.RandomState(N + len(model))
    an = _An(T=1.0, Ncut_factor=1.0)
    if model == "bsc":
        from oracle import bsc_oracle as O
        from prosper_amd.em.camodels.bsc_et import BSC_ET
        W = rng.normal(size=(D, H))
        y = (rng.random_sample((N, H)) < 0.2) @ W.T + rng.normal(size=(N, D))
        p = {"W": W + 0.1 * rng.normal(size=(D, H)), "pi": 0.4, "sigma": 1.1, "mu": np.zeros(D)}
        got = BSC_ET(D, H, Hp, gamma).step(an, dict(p), {"y": y})
        ref, log = O.em_step(O.Anneal(T=1.0, Ncut_factor=1.0, anneal_prior=False), O.make_model(D, H, Hp, gamma), dict(p), y,
                             stats_fn=O.m_step_stats_vec, vec=True)
        assert log["N_use"] == N
        np.testing.assert_allclose([got["pi"], got["sigma"]], [ref["pi"], ref["sigma"]], rtol=1e-9)      # (W: N < H, ill-posed)
    else:
        if model == "mca":
            from oracle import mca_oracle as O
            from prosper_amd.em.camodels.mca_et import MCA_ET as cls
            W = np.abs(rng.normal(size=(D, H))) * 2 + 0.1
            y = np.where((rng.random_sample((N, H)) < 0.2)[:, None, :], W[None], 0.0).max(axis=2) + rng.normal(size=(N, D))
        else:
            from oracle import mmca_oracle as O
            from prosper_amd.em.camodels.mmca_et import MMCA_ET as cls
            W = rng.normal(size=(D, H)) * 3.0
            y = O.generate_from_hidden(W, rng.random_sample((N, H)) < 0.2) + rng.normal(size=(N, D))
        m = cls(D, H, Hp, gamma)
        p = m.check_params({"W": W * (1 + 0.05 * rng.uniform(-1, 1, size=(D, H))), "pi": 0.4, "sigma": 1.1})
        got = m.step(an, dict(p), {"y": y})
        ref, log = O.em_step(O.Anneal(T=1.0, Ncut_factor=1.0), O.make_model(D, H, Hp, gamma), dict(p), y, vec=True)
        assert log["N_use"] == N
        np.testing.assert_allclose(got["W"], ref["W"], rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose([got["pi"], got["sigma"]], [ref["pi"], ref["sigma"]], rtol=1e-9)


@pytest.mark.parametrize("model", ["gsc", "dsc", "tsc", "bsc", "mca"])
def test_a_single_latent_runs(model):
    """H = H' = gamma = 1 (round 6, scratch/fuzz_shapes.py): W^T is a matrix of one row, whose stride torch reports as 1 after a
    transpose -- the Gram product was refused as "short leading dimension".  E-step against the oracle, one finite EM step."""
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU box (MI355X)")
    D, H, N = 40, 1, 50
    rng = np.random.RandomState(3)
    W = rng.normal(size=(D, H)) * 2
    if model == "gsc":
        from oracle import gsc_oracle as O
        from prosper_amd.em.camodels.gsc_et import GSC
        y = ((rng.random_sample((N, H)) < 0.4) * (1.5 + rng.normal(size=(N, H)))) @ W.T + rng.normal(size=(N, D))
        p = {"W": W.copy(), "pi": np.full(H, 0.4), "mu": np.full(H, 1.4), "psi_sq": np.eye(H) * 1.1, "sigma_sq": 1.2}
        m = GSC(D, H, 1, 1, 'scalar')
        cp = lambda q: {k: np.array(v, copy=True) for k, v in q.items()}
        d = m.select_Hprimes(cp(p), {"y": y})
        ss = m.E_step(_An(T=1.0), cp(p), d)
        suff = O.e_step(O.Anneal(T=1.0), O.make_model(D, H, 1, 1), p, y, np.asarray(d["candidates"]).astype(np.int64))
        np.testing.assert_allclose(np.asarray(ss["xpt_sz"]), suff["xpt_sz"], rtol=1e-9, atol=1e-12)
        new = m.step(_An(T=1.0), cp(p), {"y": y})
        assert np.isfinite(new["W"]).all() and np.isfinite(new["sigma_sq"])
        return
    if model in ("dsc", "tsc"):
        states = np.array([-1., 0., 1.])
        y = rng.choice(states, size=(N, H), p=[0.2, 0.6, 0.2]) @ W.T + rng.normal(size=(N, D))
        if model == "dsc":
            from oracle import dsc_oracle as O
            from prosper_amd.em.camodels.dsc_et import DSC_ET
            m, om, pi = DSC_ET(D, H, 1, 1, states=states), O.make_model(D, H, 1, 1, states), np.array([0.2, 0.6, 0.2])
        else:
            from oracle import tsc_oracle as O
            from prosper_amd.em.camodels.tsc_et import TSC_ET
            m, om, pi = TSC_ET(D, H, 1, 1), O.make_model(D, H, 1, 1), 0.4
        p = {"W": W.copy(), "pi": pi, "sigma": 1.1}
        d = m.select_Hprimes(p, {"y": y})
        ss = m.E_step(_An(T=1.0), p, d)
        ref = O.e_step_vec(O.Anneal(T=1.0, Ncut_factor=0.0, anneal_prior=False), om, p["W"], pi, 1.1, y, np.asarray(d["candidates"]))
        np.testing.assert_allclose(np.asarray(ss["logpj"]), ref, rtol=1e-10, atol=1e-9)
        new = m.step(_An(T=1.0), p, {"y": y})
    elif model == "bsc":
        from oracle import bsc_oracle as O
        from prosper_amd.em.camodels.bsc_et import BSC_ET
        y = (rng.random_sample((N, H)) < 0.4) @ W.T + rng.normal(size=(N, D))
        p = {"W": W.copy(), "pi": 0.4, "sigma": 1.1, "mu": np.zeros(D)}
        m = BSC_ET(D, H, 1, 1)
        new = m.step(_An(T=1.0), dict(p), {"y": y})
        ref, _ = O.em_step(O.Anneal(T=1.0, Ncut_factor=0.0, anneal_prior=False), O.make_model(D, H, 1, 1), dict(p), y,
                           stats_fn=O.m_step_stats_vec, vec=True)
        np.testing.assert_allclose(new["W"], ref["W"], rtol=1e-8, atol=1e-10)
    else:
        from oracle import mca_oracle as O
        from prosper_amd.em.camodels.mca_et import MCA_ET
        W = np.abs(W) + 0.1
        y = np.where((rng.random_sample((N, H)) < 0.4)[:, None, :], W[None], 0.0).max(axis=2) + rng.normal(size=(N, D))
        m = MCA_ET(D, H, 1, 1)
        p = m.check_params({"W": W.copy(), "pi": 0.4, "sigma": 1.1})
        new = m.step(_An(T=1.0), dict(p), {"y": y})
        ref, _ = O.em_step(O.Anneal(T=1.0, Ncut_factor=0.0), O.make_model(D, H, 1, 1), dict(p), y, vec=True)
        np.testing.assert_allclose(new["W"], ref["W"], rtol=1e-8, atol=1e-10)
    assert np.isfinite(np.asarray(new["W"])).all()
