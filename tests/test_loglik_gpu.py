"""log_likelihood of the component-analysis models on the device: exact by enumeration at H' = gamma = H, a bound
that tightens with H' / gamma, pinned to the reference's own ``L`` in the step goldens, per-datapoint form, repeatability,
degenerate rows, and no effect on a training run it is interleaved with."""
import itertools

import numpy as np
import pytest
from scipy.special import logsumexp

from oracle import bsc_oracle, tsc_oracle

pytestmark = pytest.mark.gpu

GOLDEN = __file__.rsplit("/", 1)[0] + "/golden/"
LOG2PI = np.log(2 * np.pi)


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def golden(name):
    return np.load(GOLDEN + name, allow_pickle=True)


def _gauss(Y, mean, var):
    """log N(y_n; mean, var I) for every row of Y and every row of mean: (N, S)."""
    D = Y.shape[1]
    r2 = ((Y[:, None, :] - mean[None, :, :]) ** 2).sum(-1)
    return -0.5 * D * np.log(2 * np.pi * var) - 0.5 * r2 / var


def _brute_binary(Y, H, log_prior_fn, mean_fn, var):
    S = np.array(list(itertools.product([0, 1], repeat=H)), dtype=np.float64)
    lp = np.array([log_prior_fn(s) for s in S])
    means = np.array([mean_fn(s) for s in S])
    return logsumexp(_gauss(Y, means, var) + lp[None, :], axis=1)


def _bsc_problem(rng, D, H, N):
    W = rng.normal(size=(D, H))
    pi, sigma = 0.3, 1.3
    s = rng.uniform(size=(N, H)) < pi
    Y = s @ W.T + sigma * rng.normal(size=(N, D))
    return {"W": W, "pi": pi, "sigma": sigma}, Y


# ---------------------------------------------------------------------------------------------------------------- 1: exact
def test_bsc_exact_by_enumeration(dev):
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    rng = np.random.RandomState(1)
    D, H, N = 9, 6, 300
    p, Y = _bsc_problem(rng, D, H, N)
    W, pi, sigma = p["W"], p["pi"], p["sigma"]
    ref = _brute_binary(Y, H, lambda s: s.sum() * np.log(pi) + (H - s.sum()) * np.log(1 - pi), lambda s: W @ s, sigma ** 2)
    m = BSC_ET(D, H, H, H)
    rows = m.log_likelihood(p, {"y": Y}, per_datapoint=True)
    np.testing.assert_allclose(rows, ref, rtol=1e-11)
    np.testing.assert_allclose(m.log_likelihood(p, {"y": Y}), ref.sum(), rtol=1e-11)
    assert "mu" not in p


@pytest.mark.parametrize("signed", [False, True], ids=["MCA", "MMCA"])
def test_mca_exact_by_enumeration(dev, signed):
    from prosper_amd.em.camodels.mca_et import MCA_ET
    from prosper_amd.em.camodels.mmca_et import MMCA_ET
    rng = np.random.RandomState(2)
    D, H, N = 9, 6, 300
    pi, sigma = 0.25, 0.7
    W = rng.uniform(-2, 3, size=(D, H)) if signed else rng.uniform(0.1, 3, size=(D, H))
    rho = 6.0 if signed else 21.0            # 1 / (1 - 1/T_rho) at T = 1: T_rho = 1.2 (MMCA), 1.05 (MCA)

    def mean(s):
        a = np.nonzero(s)[0]
        if not a.size:
            return np.zeros(D)
        Wa = W[:, a]
        if signed:
            t = (np.sign(Wa) * np.abs(Wa) ** rho).sum(axis=1)
            return np.sign(t) * np.abs(t) ** (1. / rho)
        return ((Wa ** rho).sum(axis=1)) ** (1. / rho)

    S = np.array(list(itertools.product([0, 1], repeat=H)), dtype=np.float64)
    Y = np.array([mean(S[rng.randint(len(S))]) for _ in range(N)]) + sigma * rng.normal(size=(N, D))
    ref = _brute_binary(Y, H, lambda s: s.sum() * np.log(pi) + (H - s.sum()) * np.log(1 - pi), mean, sigma ** 2)
    m = (MMCA_ET if signed else MCA_ET)(D, H, H, H)
    got = m.log_likelihood({"W": W, "pi": pi, "sigma": sigma}, {"y": Y}, per_datapoint=True)
    np.testing.assert_allclose(got, ref, rtol=1e-11)


@pytest.mark.parametrize("states", [[-1., 0., 1.], [0., 1., 2., 3.]], ids=["ternary", "K4"])
def test_dsc_exact_by_enumeration(dev, states):
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    rng = np.random.RandomState(3)
    D, H, N = 7, 4, 250
    states = np.array(states)
    K = len(states)
    pi = rng.uniform(0.5, 1.5, size=K)
    pi[list(states).index(0.)] += 4
    pi /= pi.sum()
    W, sigma = rng.normal(size=(D, H)), 0.9
    S = np.array(list(itertools.product(range(K), repeat=H)))
    lp = np.log(pi)[S].sum(axis=1)
    means = states[S] @ W.T
    Y = means[rng.randint(len(S), size=N)] + sigma * rng.normal(size=(N, D))
    ref = logsumexp(_gauss(Y, means, sigma ** 2) + lp[None, :], axis=1)
    m = DSC_ET(D, H, H, H, states=states)
    got = m.log_likelihood({"W": W, "pi": pi, "sigma": sigma}, {"y": Y}, per_datapoint=True)
    np.testing.assert_allclose(got, ref, rtol=1e-11)


def test_tsc_exact_by_enumeration(dev):
    from prosper_amd.em.camodels.tsc_et import TSC_ET
    rng = np.random.RandomState(4)
    D, H, N = 8, 5, 250
    pi, sigma = 0.3, 0.8
    W = rng.normal(size=(D, H))
    S = np.array(list(itertools.product([-1., 0., 1.], repeat=H)))
    nz = (S != 0).sum(axis=1)
    lp = nz * np.log(pi / 2) + (H - nz) * np.log(1 - pi)
    means = S @ W.T
    Y = means[rng.randint(len(S), size=N)] + sigma * rng.normal(size=(N, D))
    ref = logsumexp(_gauss(Y, means, sigma ** 2) + lp[None, :], axis=1)
    m = TSC_ET(D, H, H, H)
    got = m.log_likelihood({"W": W, "pi": pi, "sigma": sigma}, {"y": Y}, per_datapoint=True)
    # TSC's candidates are the latents of the H' best one-cause states and may repeat one (tsc_et.py:142-213): K_n is every
    # value assignment to the candidate POSITIONS, which is every state exactly when the candidates are all H latents
    cand = tsc_oracle.select_hprimes_vec(tsc_oracle.make_model(D, H, H, H), W, pi, sigma, Y)
    lpos = nz * np.log(pi / 2) + (H - nz) * np.log(1 - pi)
    pos = np.array([logsumexp(_gauss(Y[n:n + 1], S @ W[:, cand[n]].T, sigma ** 2)[0] + lpos) for n in range(N)])
    np.testing.assert_allclose(got, pos, rtol=1e-11)
    full = np.array([len(set(c)) == H for c in cand])
    assert full.sum() > N // 2
    np.testing.assert_allclose(got[full], ref[full], rtol=1e-11)


def _gsc_params(rng, D, H, kind):
    Q = rng.normal(size=(H, H)) * 0.2
    p = {"W": rng.normal(size=(D, H)), "pi": rng.uniform(0.15, 0.45, size=H), "mu": rng.normal(size=H),
         "psi_sq": np.diag(rng.uniform(0.5, 1.5, size=H)) + Q @ Q.T}
    if kind == "scalar":
        p["sigma_sq"] = np.float64(0.6)
    elif kind == "diagonal":
        p["sigma_sq"] = rng.uniform(0.3, 1.2, size=D)
    else:
        R = rng.normal(size=(D, D)) * 0.3
        p["sigma_sq"] = np.diag(rng.uniform(0.3, 1.0, size=D)) + R @ R.T
    return p


def _gsc_brute(p, Y):
    W, pi, mu, Psi = p["W"], p["pi"], p["mu"], p["psi_sq"]
    D, H = W.shape
    sig = np.asarray(p["sigma_sq"], dtype=np.float64)
    Sig = sig * np.eye(D) if sig.ndim == 0 else (np.diag(sig) if sig.ndim == 1 else sig)
    cols = []
    for s in itertools.product([0, 1], repeat=H):
        a = np.nonzero(s)[0]
        lp = np.log(pi[a]).sum() + np.log(1 - np.delete(pi, a)).sum()
        Wa = W[:, a]
        C = Sig + Wa @ Psi[np.ix_(a, a)] @ Wa.T
        r = Y - (Wa @ mu[a])[None, :]
        _, ld = np.linalg.slogdet(C)
        q = (r * np.linalg.solve(C, r.T).T).sum(axis=1)
        cols.append(lp - 0.5 * D * LOG2PI - 0.5 * ld - 0.5 * q)
    return logsumexp(np.stack(cols, axis=1), axis=1)


@pytest.mark.parametrize("kind", ["scalar", "diagonal", "full"])
def test_gsc_exact_by_enumeration(dev, kind):
    from prosper_amd.em.camodels.gsc_et import GSC
    rng = np.random.RandomState(5)
    D, H, N = 8, 5, 200
    p = _gsc_params(rng, D, H, kind)
    Y = rng.normal(size=(N, D)) * 1.5
    m = GSC(D, H, H, H, sigma_sq_type=kind)
    pi_in = p["pi"].copy()
    got = m.log_likelihood(p, {"y": Y}, per_datapoint=True)
    np.testing.assert_array_equal(p["pi"], pi_in)
    np.testing.assert_allclose(got, _gsc_brute(p, Y), rtol=1e-11)


# ------------------------------------------------------------------------------------------------------- 3: bound, monotone
def test_bsc_truncated_bound_and_monotone(dev):
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    rng = np.random.RandomState(6)
    D, H, N = 9, 7, 400
    p, Y = _bsc_problem(rng, D, H, N)
    Y = Y + 0.5 * rng.normal(size=Y.shape)
    exact = BSC_ET(D, H, H, H).log_likelihood(p, {"y": Y}, per_datapoint=True)
    prev = None
    for Hp, g in [(3, 2), (4, 3), (5, 4), (6, 5), (7, 6)]:
        v = BSC_ET(D, H, Hp, g).log_likelihood(p, {"y": Y}, per_datapoint=True)
        assert np.all(v <= exact + 1e-12 * np.abs(exact))
        if prev is not None:
            assert np.all(v >= prev - 1e-12 * np.abs(prev))
        prev = v


# ----------------------------------------------------------------------------------------- 4: pinned to the reference's L
def _golden_model(kind, g):
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    from prosper_amd.em.camodels.tsc_et import TSC_ET
    D, H, Hp, gamma = (int(g[k]) for k in ("D", "H", "Hprime", "gamma"))
    if kind == "bsc":
        return BSC_ET(D, H, Hp, gamma), {"W": g["W"], "pi": float(g["pi"]), "sigma": float(g["sigma"])}
    if kind == "dsc":
        return DSC_ET(D, H, Hp, gamma, states=g["states"]), {"W": g["W"], "pi": g["pi"], "sigma": float(g["sigma"])}
    return TSC_ET(D, H, Hp, gamma), {"W": g["W"], "pi": float(g["pi"]), "sigma": float(g["sigma"])}


@pytest.mark.parametrize("case", ["bsc_step_c1_plain", "bsc_step_c2_plain", "bsc_step_c2_fullrank", "bsc_step_h32",
                                  "bsc_step_h256", "bsc_step_shipped", "dsc_step_h64", "dsc_step_ternary",
                                  "dsc_step_shipped", "dsc_step_shipped_g5", "tsc_step_small", "tsc_step_shipped",
                                  "tsc_step_shipped_g5"])
def test_pinned_to_reference_L(dev, case):
    g = golden(case + ".npz")
    assert float(g["T"]) == 1.0 and float(g["Ncut_factor"]) == 0.0 and not bool(g["anneal_prior"])
    kind = case[:3]
    m, p = _golden_model(kind, g)
    Y = g["y"]
    N = Y.shape[0]
    H, Hp, gamma = int(g["H"]), int(g["Hprime"]), int(g["gamma"])
    if kind == "bsc":
        const = np.log(bsc_oracle.pi_gamma_factors(float(g["pi"]), H, gamma)[0])
    elif kind == "dsc":
        const = 0.0
    else:
        const = (H - Hp) * np.log(1 - float(g["pi"])) + np.log(tsc_oracle.pi_gamma_factors(float(g["pi"]), H, gamma)[0])
    F = m.log_likelihood(p, {"y": Y})
    np.testing.assert_allclose(F / N - float(g["L"]), const, rtol=1e-10, atol=1e-10 * abs(float(g["L"])))


# ------------------------------------------------------------------------------------------ 5, 6: per datapoint, repeatable
def test_per_datapoint_sum_permutation_and_repeatable(dev):
    import torch
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels._device import DeviceArray
    rng = np.random.RandomState(7)
    D, H, N = 64, 32, 3000
    p, Y = _bsc_problem(rng, D, H, N)
    m = BSC_ET(D, H, 6, 3)
    tot = m.log_likelihood(p, {"y": Y})
    rows = m.log_likelihood(p, {"y": Y}, per_datapoint=True)
    assert rows.shape == (N,) and rows.dtype == np.float64
    np.testing.assert_allclose(rows.sum(), tot, rtol=1e-12)
    perm = rng.permutation(N)
    np.testing.assert_array_equal(m.log_likelihood(p, {"y": Y[perm]}, per_datapoint=True), rows[perm])
    # the same bits on a repeated call, from a tensor and a DeviceArray too
    assert m.log_likelihood(p, {"y": Y}) == tot
    Yt = torch.from_numpy(Y).to(dev)
    assert m.log_likelihood(p, {"y": Yt}) == tot
    assert m.log_likelihood(p, {"y": DeviceArray(Yt)}) == tot
    d = BSC_ET(D, H, 6, 3)
    d.deterministic = True
    t1 = d.log_likelihood(p, {"y": Y})
    assert d.log_likelihood(p, {"y": Y}) == t1
    np.testing.assert_allclose(t1, tot, rtol=1e-12)


# ------------------------------------------------------------------------------------------------------- 8: degenerate rows
def test_nan_row_gives_nan_in_that_row_only(dev):
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.gsc_et import GSC
    rng = np.random.RandomState(8)
    p, Y = _bsc_problem(rng, 16, 8, 200)
    Y[17, 3] = np.nan
    rows = BSC_ET(16, 8, 4, 2).log_likelihood(p, {"y": Y}, per_datapoint=True)
    assert np.isnan(rows[17]) and np.isfinite(np.delete(rows, 17)).all()
    assert np.isnan(BSC_ET(16, 8, 4, 2).log_likelihood(p, {"y": Y}))
    g = _gsc_params(rng, 8, 5, "full")
    g["sigma_sq"] = g["sigma_sq"] - 10 * np.eye(8)           # not positive definite
    assert np.isnan(GSC(8, 5, 3, 2, sigma_sq_type="full").log_likelihood(g, {"y": rng.normal(size=(50, 8))}))


def test_rows_kernel_padded_rows_and_inf(dev):
    import torch
    from prosper_amd import _lib
    rng = np.random.RandomState(9)
    for N, S, ld in [(1, 1, 1), (5, 1000, 1003), (4099, 411, 416), (37, 64, 64)]:
        X = rng.normal(size=(N, ld)) * 30
        X[0, :S] = np.inf                  # a = -1/2: every entry -inf
        if N > 2:
            X[2, S // 2] = np.nan
        off = rng.normal(size=S)
        a = -0.5
        Xd = torch.from_numpy(X).to(dev)
        od = torch.from_numpy(off).to(dev)
        rows = torch.empty(N, dtype=torch.float64, device=dev)
        work = torch.empty(int(_lib.load().pm_rows_lse_work_len(N)), dtype=torch.float64, device=dev)
        tot = torch.empty(1, dtype=torch.float64, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        _lib.call("pm_rows_lse_f64", Xd.data_ptr(), ld, N, S, a, od.data_ptr(), rows.data_ptr(), work.data_ptr(),
                  tot.data_ptr(), st)
        r = rows.cpu().numpy()
        with np.errstate(invalid="ignore"):
            ref = logsumexp(a * X[:, :S] + off[None, :], axis=1)
        assert np.isneginf(r[0])
        np.testing.assert_allclose(r[1:], ref[1:], rtol=1e-13)
        if N > 2:
            assert np.isnan(r[2]) and np.isnan(float(tot.cpu()[0]))
        else:
            np.testing.assert_allclose(float(tot.cpu()[0]), r.sum(), rtol=1e-13)
    # N = 0 writes 0, and an all -inf row gives -inf
    X = torch.full((3, 8), float("-inf"), dtype=torch.float64, device=dev)
    rows = torch.empty(3, dtype=torch.float64, device=dev)
    work = torch.empty(1, dtype=torch.float64, device=dev)
    tot = torch.full((1,), 5.0, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    _lib.call("pm_rows_lse_f64", X.data_ptr(), 8, 0, 8, 1.0, None, None, work.data_ptr(), tot.data_ptr(), st)
    assert float(tot.cpu()[0]) == 0.0
    _lib.call("pm_rows_lse_f64", X.data_ptr(), 8, 3, 8, 1.0, None, rows.data_ptr(), work.data_ptr(), tot.data_ptr(), st)
    assert np.all(np.isneginf(rows.cpu().numpy())) and np.isneginf(float(tot.cpu()[0]))


# -------------------------------------------------------------------------------------------------- 7: training undisturbed
class _Anneal(dict):
    def __missing__(self, k):
        return 0.0

    def as_dict(self):
        return dict(self)


def _schedule(steps):
    from prosper_amd.em.annealing import LinearAnnealing
    a = LinearAnnealing(steps)
    a["T"] = [(0, 2.), (.7, 1.)]
    a["Ncut_factor"] = [(0, 0.), (2. / 3, 1.)]
    a["anneal_prior"] = False
    a.as_dict = lambda: {k: a[k] for k in ("T", "Ncut_factor")}
    return a


def _train(m, params, Y, Yh, steps, interleave):
    a = _schedule(steps)
    out = []
    rec = None
    for _ in range(steps):
        params = m.step(a, params, {"y": Y})
        # the step after a held-out call found the training shard where it was: no upload (same record, same device
        # buffer -- a re-upload makes a new record and a new tensor)
        now = (id(m._data), m._data.get("key"), m._data["Y"].data_ptr())
        assert rec is None or now == rec
        out.append({k: np.array(v, copy=True) for k, v in params.items()})
        if interleave:
            m.log_likelihood({k: np.array(v, copy=True) for k, v in params.items()}, {"y": Yh})
            rec = now
        a.next()
    return out


def _same_traj(a, b):
    for pa, pb in zip(a, b):
        for k in pa:
            np.testing.assert_array_equal(pa[k], pb[k], err_msg=k)


@pytest.mark.parametrize("which", ["bsc16", "mca", "gsc", "mog"])
def test_training_undisturbed(dev, which):
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    from prosper_amd.em.camodels.gsc_et import GSC
    rng = np.random.RandomState(10)
    if which == "bsc16":
        D, H, N = 256, 256, 20000
        p, Y = _bsc_problem(rng, D, H, N + 2000)
        p["pi"] = 4.0 / H
        mk = lambda: BSC_ET(D, H, 8, 4)
    elif which == "mca":
        D, H, N = 36, 12, 3000
        W = rng.uniform(0.1, 3, size=(D, H))
        Y = np.maximum((rng.uniform(size=(N + 500, H)) < 0.2)[:, :, None] * W.T[None], 0).max(axis=1)
        Y = Y + 0.5 * rng.normal(size=Y.shape)
        p = {"W": W + 0.1 * rng.uniform(size=W.shape), "pi": 0.2, "sigma": 0.6}
        mk = lambda: MCA_ET(D, H, 6, 3)
    elif which == "gsc":
        D, H, N = 24, 10, 3000
        p = _gsc_params(rng, D, H, "scalar")
        Y = rng.normal(size=(N + 500, D))
        mk = lambda: GSC(D, H, 5, 3)
    else:
        from prosper_amd.em.mixturemodels.MoG import MoG
        D, H, N = 40, 12, 3000
        Y = rng.normal(size=(N + 500, D)) + 2 * rng.normal(size=(1, D))
        p = {"W": rng.normal(size=(D, H)), "pies": np.full(H, 1.0 / H), "sigmas_sq": rng.uniform(0.5, 2.0, size=(H, D))}
        mk = lambda: MoG(D, H, sigmas_sq_type="diagonal")
    Yt, Yh = Y[:N], Y[N:]

    def det():      # (the default build's M-step atomics land in any order: only the deterministic build repeats a run bit for bit)
        m = mk()
        m.deterministic = True       # (the mixture statistics have no atomics: the attribute is unused there)
        return m
    ref = _train(det(), dict(p), Yt, Yh, 6, False)
    got = _train(det(), dict(p), Yt, Yh, 6, True)
    _same_traj(ref, got)


# ------------------------------------------------------------------------------------------------------------- 9: bars
@pytest.mark.parametrize("which", ["bsc", "mca", "mmca", "dsc", "tsc", "gsc", "mog", "mop"])
def test_bars_learned_beats_init(dev, which):
    from prosper_amd.utils.barstest import generate_bars_dict
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    from prosper_amd.em.camodels.mmca_et import MMCA_ET
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    from prosper_amd.em.camodels.tsc_et import TSC_ET
    from prosper_amd.em.camodels.gsc_et import GSC
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.em.mixturemodels.MoP import MoP
    np.random.seed(1)
    D2, H, N = 5, 10, 2000
    D = D2 * D2
    W = 10 * generate_bars_dict(H)
    mk = {"bsc": lambda: BSC_ET(D, H, 7, 4), "mca": lambda: MCA_ET(D, H, 7, 4), "mmca": lambda: MMCA_ET(D, H, 7, 4),
          "dsc": lambda: DSC_ET(D, H, 7, 4, states=np.array([0., 1., 2.])), "tsc": lambda: TSC_ET(D, H, 7, 4),
          "gsc": lambda: GSC(D, H, 7, 4), "mog": lambda: MoG(D, H, sigmas_sq_type="diagonal"), "mop": lambda: MoP(D, H)}[which]
    m = mk()
    gt = {"W": W, "pi": 2.0 / H, "sigma": 1.0}
    if which == "dsc":
        gt["pi"] = np.array([1 - 2.0 / H, 1.5 / H, 0.5 / H])
    if which == "gsc":
        gt = {"W": W, "pi": np.full(H, 2.0 / H), "mu": np.ones(H), "psi_sq": np.eye(H) * 0.1, "sigma_sq": np.float64(1.0)}
    if which in ("mog", "mop"):
        gt = {"W": W + (1.0 if which == "mop" else 0.0), "pies": np.full(H, 1.0 / H), "sigmas_sq": np.ones((H, D))}
    data = m.generate_data(gt, N + 500)
    y = np.asarray(data["y"])
    Yt, Yh = y[:N], y[N:]
    init = m.standard_init({"y": Yt})
    if which == "dsc":
        init["pi"] = np.array([0.8, 0.1, 0.1])
    F_init = m.log_likelihood(init, {"y": Yh})
    a = _schedule(50)
    params = {k: np.array(v, copy=True) for k, v in init.items()}
    while not a.finished:
        params = m.step(a, params, {"y": Yt})
        a.next()
    assert m.log_likelihood(params, {"y": Yh}) > F_init


# ------------------------------------------------------------------------------------------ 10: config 2 against the oracle
def test_config2_against_oracle(dev):
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    rng = np.random.RandomState(11)
    D, H, Hp, gamma, N = 1024, 256, 8, 4, 2000
    p, Y = _bsc_problem(rng, D, H, N)
    p["pi"] = 4.0 / H
    p["W"] = p["W"] + 0.1 * rng.normal(size=p["W"].shape)
    m = BSC_ET(D, H, Hp, gamma)
    got = m.log_likelihood(p, {"y": Y}, per_datapoint=True)
    model = bsc_oracle.make_model(D, H, Hp, gamma)
    cand = bsc_oracle.select_hprimes_vec(p["W"], Y, Hp)
    lpj = bsc_oracle.e_step_vec(bsc_oracle.Anneal(T=1.0, Ncut_factor=0.0, anneal_prior=False), p["W"], p["pi"], p["sigma"],
                                np.zeros(D), Y, cand, model["SM"], model["state_abs"])
    c = H * np.log(1 - p["pi"]) - 0.5 * D * np.log(2 * np.pi * p["sigma"] ** 2)
    np.testing.assert_allclose(got, logsumexp(lpj, axis=1) + c, rtol=1e-10)


# ------------------------------------------------------------------------------------------------ 2: mixtures against SciPy
def _mog_ref(p, Y, full):
    from scipy import stats
    H = p["W"].shape[1]
    cols = []
    for h in range(H):
        if full:
            lpdf = stats.multivariate_normal(p["W"][:, h], p["sigmas_sq"][h]).logpdf(Y).reshape(-1)
        else:
            lpdf = stats.norm(p["W"][:, h], np.sqrt(p["sigmas_sq"][h])).logpdf(Y).sum(axis=1)
        cols.append(np.log(p["pies"][h]) + lpdf)
    return logsumexp(np.stack(cols, axis=1), axis=1)


@pytest.mark.parametrize("H", [1, 64, 257])
@pytest.mark.parametrize("kind,D", [("diagonal", 1), ("diagonal", 1030), ("full", 1), ("full", 130)])
def test_mog_against_scipy(dev, kind, D, H):
    from prosper_amd.em.mixturemodels.MoG import MoG
    rng = np.random.RandomState(12 + D + H)
    N = 300
    W = rng.normal(size=(D, H))
    if kind == "diagonal":
        sig = rng.uniform(0.5, 2.0, size=(H, D))
    else:
        R = rng.normal(size=(H, D, D)) * (0.5 / np.sqrt(D))
        sig = np.einsum("hij,hkj->hik", R, R) + np.eye(D)[None] * rng.uniform(0.3, 1.0, size=(H, 1, 1))
    pies = rng.uniform(0.2, 1.0, size=H)
    pies /= pies.sum()
    p = {"W": W, "pies": pies, "sigmas_sq": sig}
    Y = W[:, rng.randint(H, size=N)].T + rng.normal(size=(N, D))
    m = MoG(D, H, sigmas_sq_type=kind)
    rows = m.log_likelihood(p, {"y": Y}, per_datapoint=True)
    np.testing.assert_allclose(rows, _mog_ref(p, Y, kind == "full"), rtol=1e-11)
    tot = m.log_likelihood(p, {"y": Y})
    np.testing.assert_allclose(tot, rows.sum(), rtol=1e-12)
    assert m.log_likelihood(p, {"y": Y}) == tot


@pytest.mark.parametrize("H", [1, 64, 257])
@pytest.mark.parametrize("D", [1, 1030])
@pytest.mark.parametrize("A", [np.nan, "set"])
def test_mop_against_scipy(dev, A, D, H):
    from scipy import stats
    from scipy.special import gammaln
    from prosper_amd.em.mixturemodels.MoP import MoP
    rng = np.random.RandomState(13 + D + H)
    N = 300
    W = rng.uniform(0.5, 6.0, size=(D, H))
    pies = rng.uniform(0.2, 1.0, size=H)
    pies /= pies.sum()
    Y = rng.poisson(W[:, rng.randint(H, size=N)].T).astype(np.float64)
    Aval = np.nan if not isinstance(A, str) else 10.0 * D
    m = MoP(D, H, A=Aval)
    rows = m.log_likelihood({"W": W, "pies": pies}, {"y": Y}, per_datapoint=True)
    X = Y if np.isnan(Aval) else m.normalize(Y)          # the data the E-step sees
    cols = np.stack([np.log(pies[h]) + (X * np.log(W[:, h]) - W[:, h] - gammaln(X + 1)).sum(axis=1) for h in range(H)],
                    axis=1)
    ref = logsumexp(cols, axis=1)
    if np.isnan(Aval):          # integer counts: the Poisson pmf itself
        ref2 = logsumexp(np.stack([np.log(pies[h]) + stats.poisson(W[:, h]).logpmf(Y).sum(axis=1) for h in range(H)],
                                  axis=1), axis=1)
        np.testing.assert_allclose(ref, ref2, rtol=1e-12)
    np.testing.assert_allclose(rows, ref, rtol=1e-11)
    np.testing.assert_allclose(m.log_likelihood({"W": W, "pies": pies}, {"y": Y}), rows.sum(), rtol=1e-12)


def test_mixture_degenerate_inputs(dev):
    from prosper_amd.em.mixturemodels.MoG import MoG
    rng = np.random.RandomState(14)
    D, H, N = 6, 3, 40
    W = rng.normal(size=(D, H))
    sig = np.stack([np.eye(D)] * H)
    Y = rng.normal(size=(N, D))
    bad = sig.copy()
    bad[1] = -np.eye(D)                                  # rejected by the Cholesky
    m = MoG(D, H, sigmas_sq_type="full")
    assert np.isnan(m.log_likelihood({"W": W, "pies": np.full(H, 1.0 / H), "sigmas_sq": bad}, {"y": Y}))
    rows = m.log_likelihood({"W": W, "pies": np.array([0.5, 0.0, 0.5]), "sigmas_sq": bad}, {"y": Y}, per_datapoint=True)
    assert np.isfinite(rows).all()                       # (pies_h = 0: that component contributes nothing)
    Y[7, 2] = np.nan
    for kind, s in (("full", sig), ("diagonal", np.ones((H, D)))):
        rows = MoG(D, H, sigmas_sq_type=kind).log_likelihood({"W": W, "pies": np.full(H, 1.0 / H), "sigmas_sq": s}, {"y": Y},
                                                             per_datapoint=True)
        assert np.isnan(rows[7]) and np.isfinite(np.delete(rows, 7)).all()


# ------------------------------------------------------------------------------------------------------ two ranks over gloo
def test_two_ranks_over_gloo(dev):
    """tests/loglik_world2_gpu_worker.py: two processes, a world_size-2 gloo group; both ranks return the same bits, equal
    to the single-process total within 1e-12."""
    import os
    import socket
    import subprocess
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import loglik_world2_gpu_worker as w
    D, H, Y, probs = w.problems()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for kind, p in probs:
        env["LL_REF_" + kind.upper()] = repr(float(_single(w, kind, D, H, p, Y)))
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    procs = []
    for rank in range(2):
        e = dict(env, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2")
        procs.append(subprocess.Popen([sys.executable, w.__file__], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                      text=True))
    outs = []
    try:
        for pr in procs:
            outs.append(pr.communicate(timeout=300))
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
    for rank, (pr, (out, err)) in enumerate(zip(procs, outs)):
        assert pr.returncode == 0 and ("ok %d" % rank) in out.split("\n"), "rank %d\n%s\n%s" % (rank, out[-2000:], err[-4000:])


def _single(w, kind, D, H, p, Y):
    from prosper_amd.utils import parallel
    return w.make(kind, D, H, parallel.COMM_WORLD).log_likelihood(p, {"y": Y})
