"""reconstruct() on the device: against NumPy enumeration of every state at H' = gamma = H, against the E-step's
own log-joints on truncated state sets (shipped bars settings and larger shapes), the mixtures against the NumPy softmax,
that denoising denoises, that a training run is undisturbed, bit for bit repeatable, at the edges and limits, on two ranks.
NumPy references: tests/recon_reference.py (pinned on the CPU by tests/test_reconstruct_cpu.py).

Tolerance (|delta| / max_d |yhat_nd| per row, the largest over the rows): both sides are f64 and differ by summation order
only, so the project's bound for per-row values against NumPy, 1e-11 (tests/test_loglik_exact_gpu.py), holds for every
model; the measured deviations on the MI355X are recorded in DESIGN 4.14."""
import numpy as np
import pytest

import recon_reference as R

pytestmark = pytest.mark.gpu

RTOL = 1e-11


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _check(tag, got, want, rtol=RTOL):
    err = R.row_rel_err(got, want)
    print("reconstruct %-28s row-relative error %.3e (bound %.1e)" % (tag, err, rtol))
    assert got.shape == want.shape and got.dtype == np.float64
    assert err <= rtol, (tag, err)


def _mse(a, b):
    return float(((a - b) ** 2).mean())


# ------------------------------------------------------------------------------------------------ problems per model
def _gsc_params(rng, D, H, kind):
    Q = rng.normal(size=(H, H)) * 0.2
    p = {"W": rng.normal(size=(D, H)), "pi": rng.uniform(0.15, 0.45, size=H), "mu": rng.normal(size=H),
         "psi_sq": np.diag(rng.uniform(0.5, 1.5, size=H)) + Q @ Q.T}
    if kind == "scalar":
        p["sigma_sq"] = np.float64(0.6)
    elif kind == "diagonal":
        p["sigma_sq"] = rng.uniform(0.3, 1.2, size=D)
    else:
        Rm = rng.normal(size=(D, D)) * 0.3
        p["sigma_sq"] = np.diag(rng.uniform(0.3, 1.0, size=D)) + Rm @ Rm.T
    return p


def _problem(name, rng, D, H, N, Hp, g):
    """(model, params, Y, noiseless means, NumPy enumeration fn(Y)): data drawn from the parameters the call is given."""
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    from prosper_amd.em.camodels.mmca_et import MMCA_ET
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    from prosper_amd.em.camodels.tsc_et import TSC_ET
    from prosper_amd.em.camodels.gsc_et import GSC
    if name in ("bsc", "bsc_mu"):
        W, pi, sigma = rng.normal(size=(D, H)), 0.3, 1.3
        p = {"W": W, "pi": pi, "sigma": sigma}
        mu = None
        if name == "bsc_mu":
            mu = p["mu"] = rng.normal(size=D)
        clean = (rng.uniform(size=(N, H)) < pi) @ W.T + (0.0 if mu is None else mu)
        Y = clean + sigma * rng.normal(size=(N, D))
        return BSC_ET(D, H, Hp, g), p, Y, clean, lambda Y: R.enum_linear(Y, W, sigma, [0., 1.], np.log([1 - pi, pi]), mu=mu)
    if name in ("mca", "mmca"):
        signed = name == "mmca"
        W = rng.uniform(-2, 3, size=(D, H)) if signed else rng.uniform(0.1, 3, size=(D, H))
        W = np.where(np.abs(W) < 0.05, 0.05, W)
        pi, sigma = 0.25, 0.7
        rho = 6.0 if signed else 21.0
        mean = R.mca_mean(W, rho, signed)
        S = rng.uniform(size=(N, H)) < pi
        clean = np.array([mean(np.nonzero(s)[0]) for s in S])
        Y = clean + sigma * rng.normal(size=(N, D))
        m = (MMCA_ET if signed else MCA_ET)(D, H, Hp, g)
        return m, {"W": W, "pi": pi, "sigma": sigma}, Y, clean, lambda Y: R.enum_mca(Y, W, rho, signed, pi, sigma)
    if name.startswith("dsc"):
        states = np.array({"dsc3": [-1., 0., 1.], "dsc8": [-3., -2., -1., 0., 1., 2., 3., 4.]}.get(name, [0., 1., 2., 3.]))
        K = len(states)
        pi = rng.uniform(0.5, 1.5, size=K)
        pi[list(states).index(0.)] += 4
        pi /= pi.sum()
        W, sigma = rng.normal(size=(D, H)), 0.9
        clean = states[rng.choice(K, p=pi, size=(N, H))] @ W.T
        Y = clean + sigma * rng.normal(size=(N, D))
        return (DSC_ET(D, H, Hp, g, states=states), {"W": W, "pi": pi, "sigma": sigma}, Y, clean,
                lambda Y: R.enum_linear(Y, W, sigma, states, np.log(pi)))
    if name == "tsc":
        W, pi, sigma = rng.normal(size=(D, H)), 0.3, 0.8
        S = rng.choice(3, p=[pi / 2, 1 - pi, pi / 2], size=(N, H)) - 1.
        clean = S @ W.T
        Y = clean + sigma * rng.normal(size=(N, D))
        return (TSC_ET(D, H, Hp, g), {"W": W, "pi": pi, "sigma": sigma}, Y, clean,
                lambda Y: R.enum_linear(Y, W, sigma, [-1., 0., 1.], np.log([pi / 2, 1 - pi, pi / 2])))
    kind = name.split("_")[1]
    p = _gsc_params(rng, D, H, kind)
    p["pi"] = p["pi"] * min(1.0, 8.0 / H)       # about as many active latents at every H: a truncated state set fits the data
    S = rng.uniform(size=(N, H)) < p["pi"][None, :]
    Lp = np.linalg.cholesky(p["psi_sq"])
    clean = np.zeros((N, D))
    for n in range(N):
        a = np.nonzero(S[n])[0]
        if a.size:
            La = np.linalg.cholesky(p["psi_sq"][np.ix_(a, a)])
            clean[n] = p["W"][:, a] @ (p["mu"][a] + La @ rng.normal(size=a.size))
    Sig = R._gsc_sigma(p, D)
    Y = clean + rng.normal(size=(N, D)) @ np.linalg.cholesky(Sig).T
    return GSC(D, H, Hp, g, sigma_sq_type=kind), p, Y, clean, lambda Y: R.enum_gsc(p, Y)


ENUM = ["bsc", "bsc_mu", "mca", "mmca", "dsc3", "dsc4", "tsc", "gsc_scalar", "gsc_diagonal", "gsc_full"]
# (name: D, H, seed) -- tsc: (12, 6) with RandomState(1) keeps 221 of its 300 rows (distinct candidates)
ENUM_SHAPE = {"bsc": (25, 8, 101), "bsc_mu": (16, 7, 102), "mca": (12, 6, 103), "mmca": (14, 6, 104), "dsc3": (12, 6, 105),
              "dsc4": (13, 6, 106), "tsc": (12, 6, 1), "gsc_scalar": (12, 6, 108), "gsc_diagonal": (15, 6, 109),
              "gsc_full": (12, 7, 110)}


def _tsc_distinct(p, Y, D, H):
    from oracle import tsc_oracle
    cand = tsc_oracle.select_hprimes_vec(tsc_oracle.make_model(D, H, H, H), p["W"], p["pi"], p["sigma"], Y)
    return np.array([len(set(c)) == H for c in cand])


# --------------------------------------------------------------------------- 1 + 4: against enumeration; denoising denoises
@pytest.mark.parametrize("name", ENUM)
def test_against_enumeration_and_denoises(dev, name):
    D, H, seed = ENUM_SHAPE[name]
    N = 300
    m, p, Y, clean, enum = _problem(name, np.random.RandomState(seed), D, H, N, H, H)
    p_in = {k: np.array(v, copy=True) for k, v in p.items()}
    want = enum(Y)
    got = m.reconstruct(p, {"y": Y})
    assert got.shape == (N, D) and got.dtype == np.float64
    for k in p_in:
        np.testing.assert_array_equal(p[k], p_in[k])
    assert set(p) == set(p_in) and (m.Hprime, m.gamma) == (H, H)
    keep = np.ones(N, dtype=bool)
    if name == "tsc":              # rows whose candidates repeat a latent hold pseudo-states: not the model's posterior
        keep = _tsc_distinct(p, Y, D, H)
        assert keep.sum() >= N // 2, keep.sum()
    _check(name, got[keep], want[keep])
    # the exact posterior mean is the minimum-mean-square estimate: first on the NumPy reference (a failure there blames
    # the inputs), then on the device output
    noisy = _mse(Y[keep], clean[keep])
    assert _mse(want[keep], clean[keep]) < noisy
    assert _mse(got[keep], clean[keep]) < noisy
    print("reconstruct %-28s MSE noisy %.4f -> reconstructed %.4f" % (name, noisy, _mse(got[keep], clean[keep])))


# ----------------------------------------------------------------- 2: against the E-step's own log-joints, truncated
def _truncated_reference(m, name, p, Y):
    """q and ybar in NumPy from ``compute_lpj``'s (logpj, candidates) -- GSC: from the doubled-logit pass ``_loglik_terms``
    reads, with NumPy kappa."""
    from prosper_amd.em.camodels._device import LoglikPoint
    H = m.H
    if name.startswith("gsc"):
        saved = m._eval_begin()
        try:
            m._lpi_scale = 2.0
            lp, cand = m.compute_lpj(None, dict(p), {"y": Y})
            lp, cand = np.asarray(lp), np.asarray(cand)
        finally:
            m._eval_end(saved)
        # ordinary data: no row whose weights all underflow (the E-step pass floors a weight at DBL_MIN)
        assert (0.5 * lp).max(axis=1).min() > -650.0
        return R.gsc_from_lpj(p, Y, lp, cand, m.state_matrix)
    lp, cand = m.compute_lpj(LoglikPoint(), dict(p), {"y": Y})
    lp, cand = np.asarray(lp), np.asarray(cand)
    if name in ("mca", "mmca"):
        return R.mca_from_lpj(lp, cand, m.state_matrix, p["W"], m._rho(1.0), name == "mmca")
    if name.startswith("bsc"):
        return R.linear_from_lpj(lp, 1.0, cand, p["W"], (1.0,), 1, 1 + H, m.state_matrix, mu=p.get("mu"))
    if name.startswith("dsc"):
        blocks = [v for v in m.states if v != 0.]
        return R.linear_from_lpj(lp, 1.0, cand, p["W"], blocks, 1, 1 + len(blocks) * H, m.state_matrix)
    return R.linear_from_lpj(lp, 1.0, cand, p["W"], (), 0, 0, m.state_matrix)


# shipped bars settings (D = 25, H = 10) and one larger shape per model
TRUNC = [("bsc", 25, 10, 8, 5), ("bsc_mu", 25, 10, 8, 5), ("mca", 25, 10, 8, 5), ("mmca", 25, 10, 7, 5), ("dsc3", 25, 10, 7, 5),
         ("tsc", 25, 10, 7, 5), ("gsc_scalar", 25, 10, 7, 4),
         ("bsc", 256, 128, 6, 3), ("bsc_mu", 64, 40, 8, 4), ("mca", 64, 32, 10, 3), ("mmca", 96, 24, 8, 3),
         ("dsc4", 64, 32, 6, 3), ("tsc", 64, 32, 5, 3), ("gsc_diagonal", 48, 24, 6, 3), ("gsc_full", 40, 16, 5, 3)]
# one case per branch of the two kernels that the shapes above leave out (test -> branch in DESIGN 4.14):
#   recon_mca_kernel<DPL>   D = 200, 400 and 500, 1000: DPL 4, 8, 16 (the shapes above: 1 and 2); 200, 500 and 1000 reach the
#                           lane's last slab of 64 dimensions (D > 64 (DPL - 1)), 400 leaves the last of its eight empty
#   recon_expect_kernel     H' = 16 (PM_MAX_HPRIME; above: <= 10); DSC with H = 130 > 64 (the lane-strided H loop over
#                           soff + c H + h, three blocks) at H' = 12; TSC with H = 70 (repeated candidates, H > 64); a DSC
#                           model of 8 latent values: nblk = 7 blocks
TRUNC_MORE = [(k, D, 24, 6, 3) for k in ("mca", "mmca") for D in (200, 400, 1000)] + [("mca", 500, 24, 6, 3)] + \
             [("bsc", 40, 48, 16, 2), ("dsc4", 24, 130, 12, 2), ("tsc", 24, 70, 5, 3), ("dsc8", 16, 12, 3, 2)]


def _entries(m):
    """The model's launch hook, wrapped to keep the names of the entry points that ran."""
    calls = []
    orig = m._call
    m._call = lambda label, entry, *args: (calls.append(entry), orig(label, entry, *args))[1]
    return calls


@pytest.mark.parametrize("name,D,H,Hp,g", TRUNC + TRUNC_MORE)
def test_against_the_esteps_log_joints(dev, name, D, H, Hp, g):
    N = 160 if (name, D, H, Hp, g) in TRUNC else 96
    m, p, Y, _, _ = _problem(name, np.random.RandomState(D + H + Hp), D, H, N, Hp, g)
    if name in ("mca", "mmca"):
        p = m.check_params({k: np.array(v, copy=True) for k, v in p.items()})
    want = _truncated_reference(m, name, p, Y)
    calls = _entries(m)
    got = m.reconstruct(p, {"y": Y})
    if not name.startswith("gsc"):
        assert "pm_recon_expect_f64" in calls and ("pm_recon_mca_f64" in calls) == (name in ("mca", "mmca")), calls
    _check("%s D=%d H=%d H'=%d g=%d" % (name, D, H, Hp, g), got, want)


# the second trip of the kernels' grid-stride loops: both launch at most REC_MAX_BLOCKS = 8192 workgroups of four rows
@pytest.mark.parametrize("name", ["bsc", "mca", "dsc3"])
def test_second_trip_of_the_row_loops(dev, name):
    """N = 32768 + 77: every wavefront of the first 77 / 4 workgroups takes a second row.  The rows from 150 before the
    boundary to the end against the NumPy sums over an E-step of those rows alone; the whole result bit for bit against
    the same call on shards of 4096 rows (rows are independent and a row's sums run in a fixed order)."""
    D, H, Hp, g, N = 8, 6, 4, 2, 32768 + 77
    m, p, Y, _, _ = _problem(name, np.random.RandomState(900 + len(name)), D, H, N, Hp, g)
    if name == "mca":
        p = m.check_params({k: np.array(v, copy=True) for k, v in p.items()})
    got = m.reconstruct(p, {"y": Y})
    assert got.shape == (N, D) and np.isfinite(got).all()
    tail = slice(32768 - 150, N)
    _check("%s second trip" % name, got[tail], _truncated_reference(m, name, p, Y[tail]))
    shards = np.concatenate([m.reconstruct(p, {"y": Y[i:i + 4096]}) for i in range(0, N, 4096)])
    assert np.array_equal(shards.view(np.uint64), got.view(np.uint64))


def test_bsc_fallback_path_past_512_latents(dev):
    """H > 512: the E-step's fallback kernels write the log-joints; reconstruct consumes them all the same."""
    D, H, Hp, g, N = 24, 520, 5, 2, 70
    m, p, Y, _, _ = _problem("bsc_mu", np.random.RandomState(77), D, H, N, Hp, g)
    p["pi"] = 2.0 / H
    want = _truncated_reference(m, "bsc_mu", p, Y)
    _check("bsc H=520", m.reconstruct(p, {"y": Y}), want)


def _mixture(kind, rng, D, H, N):
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.em.mixturemodels.MoP import MoP
    pies = rng.uniform(0.5, 1.5, size=H)
    pies /= pies.sum()
    z = rng.choice(H, p=pies, size=N)
    if kind.startswith("mop"):
        A = 3.0 * D if kind == "mop_A" else np.nan
        m = MoP(D, H, A=A) if kind == "mop_A" else MoP(D, H)
        W = rng.uniform(0.5, 6.0, size=(D, H))
        if kind == "mop_A":
            W = W / W.sum(0)[None, :] * A
        Y = rng.poisson(W.T[z]).astype(np.float64)
        X = m.normalize(Y) if kind == "mop_A" else Y
        p = {"W": W, "pies": pies}
        return m, p, Y, R.mop_recon(X, W, pies)
    full = kind == "mog_full"
    m = MoG(D, H, sigmas_sq_type="full" if full else "diagonal")
    W = rng.normal(size=(D, H)) * 2
    if full:
        sig = np.stack([np.diag(rng.uniform(0.5, 2.0, size=D)) + 0.1 * np.outer(v, v) for v in rng.normal(size=(H, D))])
    else:
        sig = rng.uniform(0.5, 2.0, size=(H, D))
    Y = W.T[z] + rng.normal(size=(N, D))
    p = {"W": W, "pies": pies, "sigmas_sq": sig}
    return m, p, Y, R.mog_recon(Y, W, pies, sig)


MIX = ["mog_diagonal", "mog_full", "mop", "mop_A"]


@pytest.mark.parametrize("kind", MIX)
@pytest.mark.parametrize("D,H", [(10, 6), (40, 21)])
def test_mixtures_against_numpy_softmax(dev, kind, D, H):
    m, p, Y, want = _mixture(kind, np.random.RandomState(D + len(kind)), D, H, 250)
    p_in = {k: np.array(v, copy=True) for k, v in p.items()}
    got = m.reconstruct(p, {"y": Y})
    _check("%s D=%d H=%d" % (kind, D, H), got, want)
    for k in p_in:
        np.testing.assert_array_equal(p[k], p_in[k])


# ------------------------------------------------------------------------------------------- 5: training undisturbed
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
    for _ in range(steps):
        params = m.step(a, params, {"y": Y})
        if interleave:
            hp = (getattr(m, "Hprime", None), getattr(m, "gamma", None))
            out = m.reconstruct({k: np.array(v, copy=True) for k, v in params.items()}, {"y": Yh})
            assert out.shape == Yh.shape and np.isfinite(out).all()
            assert (getattr(m, "Hprime", None), getattr(m, "gamma", None)) == hp
        a.next()
    return {k: np.array(v, copy=True) for k, v in params.items()}, getattr(m, "spec_hits", None)


@pytest.mark.parametrize("name", ["bsc", "mca", "mmca", "dsc3", "tsc", "gsc_scalar", "mog_diagonal", "mog_full", "mop"])
def test_training_undisturbed(dev, name):
    rng = np.random.RandomState(14)
    N, Nh = 1500, 300
    if name.startswith("mo"):
        D, H = 12, 5
        _, p, Y, _ = _mixture(name, rng, D, H, N + Nh)
        mk = lambda: _mixture(name, np.random.RandomState(0), D, H, 4)[0]
        p = dict(p, W=p["W"] * rng.uniform(0.9, 1.1, size=p["W"].shape))
    else:
        D, H = 20, 10
        _, p, Y, _, _ = _problem(name, rng, D, H, N + Nh, 5, 3)
        mk = lambda: _problem(name, np.random.RandomState(0), D, H, 4, 5, 3)[0]
        p = dict(p, W=p["W"] * rng.uniform(0.9, 1.1, size=p["W"].shape))
    Yt, Yh = Y[:N], Y[N:]

    def det():
        m = mk()
        m.deterministic = True
        return m
    ref, hits_ref = _train(det(), {k: np.array(v, copy=True) for k, v in p.items()}, Yt, Yh, 6, False)
    got, hits_got = _train(det(), {k: np.array(v, copy=True) for k, v in p.items()}, Yt, Yh, 6, True)
    for k in ref:
        np.testing.assert_array_equal(ref[k], got[k], err_msg=k)
    if name in ("bsc", "gsc_scalar"):
        assert hits_ref is not None and hits_ref == hits_got, (hits_ref, hits_got)


# ------------------------------------------------------------------------------------------------------------ 6: bits
@pytest.mark.parametrize("name", ["bsc_mu", "mca", "mmca", "dsc4", "tsc", "gsc_scalar", "gsc_full", "mog_diagonal", "mog_full",
                                  "mop_A"])
def test_bits_repeat_across_calls_builds_row_order_and_device_output(dev, name):
    from prosper_amd.em.camodels._device import DeviceArray
    rng = np.random.RandomState(13)
    if name.startswith("mo"):
        m, p, Y, _ = _mixture(name, rng, 24, 9, 700)
    else:
        m, p, Y, _, _ = _problem(name, rng, 24, 12, 700, 5, 3)
    a = m.reconstruct(p, {"y": Y})
    np.testing.assert_array_equal(m.reconstruct(p, {"y": Y}), a)
    d = m.reconstruct(p, {"y": Y}, device=True)
    assert isinstance(d, DeviceArray) and d.tensor.is_cuda
    np.testing.assert_array_equal(np.asarray(d), a)
    if hasattr(m, "deterministic") and name != "gsc_full":      # (GSC's deterministic mode is built for a scalar sigma_sq)
        m.deterministic = True
        np.testing.assert_array_equal(m.reconstruct(p, {"y": Y}), a)
        m.deterministic = False
    perm = rng.permutation(len(Y))
    np.testing.assert_array_equal(m.reconstruct(p, {"y": Y[perm]}), a[perm])
    import torch
    np.testing.assert_array_equal(m.reconstruct(p, {"y": torch.from_numpy(Y).to(dev)}), a)
    np.testing.assert_array_equal(m.reconstruct(p, {"y": DeviceArray(torch.from_numpy(Y).to(dev))}), a)


# ----------------------------------------------------------------------------------------------------------- 7: edges
@pytest.mark.parametrize("name", ["bsc", "mca", "mmca", "dsc3", "tsc", "gsc_full", "mog_diagonal", "mog_full", "mop"])
def test_nan_row_and_empty(dev, name):
    rng = np.random.RandomState(11)
    if name.startswith("mo"):
        m, p, Y, _ = _mixture(name, rng, 6, 5, 70)
    else:
        m, p, Y, _, _ = _problem(name, rng, 6, 5, 70, 3, 2)
    clean_rows = m.reconstruct(p, {"y": np.delete(Y, 13, axis=0)})
    Y = Y.copy()
    Y[13, 2] = np.nan
    rows = m.reconstruct(p, {"y": Y})
    assert np.isnan(rows[13]).all() and np.isfinite(np.delete(rows, 13, axis=0)).all()
    np.testing.assert_array_equal(np.delete(rows, 13, axis=0), clean_rows)
    calls = []
    if hasattr(m, "_call"):
        orig = m._call
        m._call = lambda label, entry, *args: (calls.append(entry), orig(label, entry, *args))[1]
    empty = m.reconstruct(p, {"y": np.zeros((0, 6))})
    assert empty.shape == (0, 6) and empty.dtype == np.float64 and not calls
    assert m.reconstruct(p, {"y": np.zeros((0, 6))}, device=True).shape == (0, 6)


@pytest.mark.parametrize("pi", [0.0, 1.0])
def test_bsc_tsc_prior_at_zero_and_one(dev, pi):
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.tsc_et import TSC_ET
    rng = np.random.RandomState(8)
    D, H, N = 6, 5, 40
    W, sigma = rng.normal(size=(D, H)), 0.9
    Y = rng.normal(size=(N, D))
    p = {"W": W, "pi": pi, "sigma": sigma}
    if pi == 0.0:
        np.testing.assert_array_equal(BSC_ET(D, H, H, H).reconstruct(p, {"y": Y}), np.zeros((N, D)))
    else:
        # BSC's E-step works with the prior odds pi / (1 - pi) (bsc_et.py:160-166): pi = 1 has no log-joints there, and
        # reconstruct, which consumes them, has no value either -- the call raises as the E-step does, it returns no NaN
        with pytest.raises(ZeroDivisionError):
            BSC_ET(D, H, H, H).reconstruct(p, {"y": Y})
    tsc = TSC_ET(D, H, H, H).reconstruct(p, {"y": Y})
    assert np.isfinite(tsc).all()
    if pi == 0.0:
        np.testing.assert_array_equal(tsc, np.zeros((N, D)))
    else:
        keep = _tsc_distinct(p, Y, D, H)
        assert keep.any()
        want = R.enum_linear(Y, W, sigma, [-1., 1.], np.log([0.5, 0.5]))
        _check("tsc pi=1", tsc[keep], want[keep])


def test_dsc_value_of_zero_prior(dev):
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    rng = np.random.RandomState(9)
    D, H, N = 6, 4, 50
    states = np.array([0., 1., 2., 3.])
    pi = np.array([0.6, 0.25, 0.0, 0.15])
    W, sigma = rng.normal(size=(D, H)), 0.8
    Y = rng.normal(size=(N, D)) * 2
    got = DSC_ET(D, H, H, H, states=states).reconstruct({"W": W, "pi": pi, "sigma": sigma}, {"y": Y})
    assert np.isfinite(got).all()
    with np.errstate(divide="ignore"):
        _check("dsc pi_k=0", got, R.enum_linear(Y, W, sigma, states, np.log(pi)))


def test_indefinite_covariances_give_nan_rows(dev):
    from prosper_amd.em.camodels.gsc_et import GSC
    from prosper_amd.em.mixturemodels.MoG import MoG
    rng = np.random.RandomState(12)
    D, H = 5, 4
    p = _gsc_params(rng, D, H, "full")
    p["sigma_sq"] = np.diag([1., 1., -0.5, 1., 1.])
    rows = GSC(D, H, 2, 2, sigma_sq_type="full").reconstruct(p, {"y": rng.normal(size=(9, D))})
    assert rows.shape == (9, D) and np.isnan(rows).all()
    sig = np.stack([np.eye(D)] * H)
    sig[2] = np.diag([1., -1., 1., 1., 1.])
    q = {"W": rng.normal(size=(D, H)), "pies": np.full(H, 1.0 / H), "sigmas_sq": sig}
    rows = MoG(D, H, sigmas_sq_type="full").reconstruct(q, {"y": rng.normal(size=(9, D))})
    assert rows.shape == (9, D) and np.isnan(rows).all()


def test_limits_raise_hip_error(dev):
    from prosper_amd import _lib
    from prosper_amd.em.camodels.mca_et import MCA_ET
    rng = np.random.RandomState(5)
    D, H = 1025, 8
    p = {"W": rng.uniform(0.5, 2.0, size=(D, H)), "pi": 0.2, "sigma": 1.0}
    with pytest.raises(_lib.HipError):
        MCA_ET(D, H, 4, 2).reconstruct(p, {"y": rng.uniform(0, 2, size=(5, D))})


def test_at_and_one_past_the_candidate_and_latent_limits(dev):
    """PM_MAX_HPRIME = 16 runs (TRUNC_MORE), 17 raises; BSC with PM_MAX_H = 1024 latents runs, 1025 raises -- HipError from
    the library or from the constructor's own range check, before any row is produced."""
    from prosper_amd import _lib
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    rng = np.random.RandomState(6)
    D, N = 16, 48
    for H, Hp, ok in ((1024, 4, True), (1025, 4, False), (40, 17, False)):
        p = {"W": rng.normal(size=(D, H)), "pi": 2.0 / H, "sigma": 1.0}
        Y = rng.normal(size=(N, D))
        if ok:
            m = BSC_ET(D, H, Hp, 2)
            _check("bsc H=%d" % H, m.reconstruct(p, {"y": Y}), _truncated_reference(m, "bsc", p, Y))
        else:
            with pytest.raises(_lib.HipError):
                BSC_ET(D, H, Hp, 2).reconstruct(p, {"y": Y})


# ------------------------------------------------------------------------------------------------------- 8: two ranks
def test_two_ranks_over_gloo(dev):
    """tests/reconstruct_world2_gpu_worker.py: two processes, a world_size-2 gloo group on the one GPU; each rank's rows
    equal the corresponding rows of a one-rank call, bit for bit."""
    import os
    import socket
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    worker = os.path.join(here, "reconstruct_world2_gpu_worker.py")
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    procs = []
    for rank in range(2):
        e = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                 RANK=str(rank), WORLD_SIZE="2")
        procs.append(subprocess.Popen([sys.executable, worker], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
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
