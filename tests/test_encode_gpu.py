"""encode() on the device, all eight models: against the NumPy reference on the E-step's own log-joints
(shipped bars settings and one larger shape per model), against NumPy enumeration of every state at H' = gamma = H, against
reconstruct(), exact=True, masks and weights, bit for bit repeatable, with a training run undisturbed, at the limits.
NumPy references: tests/encode_reference.py (pinned on the CPU by tests/test_encode_cpu.py); problems per model:
tests/test_reconstruct_gpu.py.

Tolerance: |delta| relative to the largest entry of the row, the largest over the rows (recon_reference.row_rel_err), at most
1e-11 -- the bound tests/test_reconstruct_gpu.py holds the same read-out to: both sides are f64 and differ by summation order
only.  exact=True against the truncated path at H' = gamma = H: 2e-11, each side being within 1e-11 of the truth."""
import numpy as np
import pytest

import encode_reference as E
import recon_reference as R
from test_reconstruct_gpu import ENUM_SHAPE, MIX, RTOL, TRUNC, _entries, _mixture, _problem, _schedule, _tsc_distinct

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _check(tag, got, want, rtol=RTOL):
    for what, g, w in zip(("mean", "prob"), got, want):
        err = R.row_rel_err(g, w)
        print("encode %-30s %s row-relative error %.3e (bound %.1e)" % (tag, what, err, rtol))
        assert g.shape == w.shape and g.dtype == np.float64
        assert err <= rtol, (tag, what, err)


def _bits(a, b, what=""):
    for x, y in zip(a, b):
        x, y = np.ascontiguousarray(np.asarray(x)), np.ascontiguousarray(np.asarray(y))
        assert x.shape == y.shape and x.dtype == y.dtype == np.float64, what
        assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), what


def _copy(p):
    return {k: np.array(v, copy=True) for k, v in p.items()}


def _in_range(pair, binary=False):
    mean, prob = pair
    assert np.isfinite(mean).all() and prob.min() >= 0.0 and prob.max() <= 1.0
    if binary:                                   # prob = min(mean, 1): the same bits wherever no sum rounds above 1
        assert np.array_equal(prob.view(np.uint64), np.minimum(mean, 1.0).view(np.uint64))


BINARY = ("bsc", "bsc_mu", "mca", "mmca")


# ----------------------------------------------------------------- 1: against the E-step's own log-joints, truncated
def _truncated_reference(m, name, p, Y):
    """(mean, prob) in NumPy from ``compute_lpj``'s (logpj, candidates) -- GSC: from the doubled-logit pass."""
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
        return E.gsc_from_lpj(p, Y, lp, cand, m.state_matrix)
    lp, cand = m.compute_lpj(LoglikPoint(), dict(p), {"y": Y})
    lp, cand = np.asarray(lp), np.asarray(cand)
    if name in BINARY:
        return E.codes_from_lpj(lp, 1.0, cand, H, (1.0,), 1, 1 + H, m.state_matrix if m.no_states else None)
    if name.startswith("dsc"):
        blocks = [v for v in m.states if v != 0.]
        return E.codes_from_lpj(lp, 1.0, cand, H, blocks, 1, 1 + len(blocks) * H, m.state_matrix if m.no_states else None)
    return E.codes_from_lpj(lp, 1.0, cand, H, (), 0, 0, m.state_matrix)


@pytest.mark.parametrize("name,D,H,Hp,g", TRUNC)
def test_against_the_esteps_log_joints(dev, name, D, H, Hp, g):
    N = 160
    m, p, Y, _, _ = _problem(name, np.random.RandomState(D + H + Hp), D, H, N, Hp, g)
    if name in ("mca", "mmca"):
        p = m.check_params(_copy(p))
    want = _truncated_reference(m, name, p, Y)
    p_in = _copy(p)
    calls = _entries(m)
    got = m.encode(p, {"y": Y})
    assert isinstance(got, tuple) and len(got) == 2 and got[0].shape == got[1].shape == (N, H)
    for k in p_in:
        np.testing.assert_array_equal(p[k], p_in[k])
    assert set(p) == set(p_in) and (m.Hprime, m.gamma) == (Hp, g)
    if name.startswith("gsc"):
        assert "pm_encode_f64" not in calls and any("gsc_estep" in c for c in calls), calls
    else:
        assert "pm_encode_f64" in calls and "pm_recon_expect_f64" not in calls and "pm_recon_mca_f64" not in calls, calls
    _check("%s D=%d H=%d H'=%d g=%d" % (name, D, H, Hp, g), got, want)
    _in_range(got, name in BINARY)


def _mixture_reference(kind, m, p, Y):
    X = m.normalize(Y) if kind == "mop_A" else Y
    return E.mixture_resp(kind, X, p["W"], p["pies"], p.get("sigmas_sq"))


@pytest.mark.parametrize("kind", MIX)
@pytest.mark.parametrize("D,H", [(10, 6), (40, 21)])
def test_mixtures_against_numpy_responsibilities(dev, kind, D, H):
    m, p, Y, _ = _mixture(kind, np.random.RandomState(D + len(kind)), D, H, 250)
    p_in = _copy(p)
    got = m.encode(p, {"y": Y})
    want = _mixture_reference(kind, m, p, Y)
    _check("%s D=%d H=%d" % (kind, D, H), got, (want, want))
    _in_range(got, True)
    for k in p_in:
        np.testing.assert_array_equal(p[k], p_in[k])
    _bits(m.encode(p, {"y": Y}, exact=True), got, "exact=True returns the same bits")


# ------------------------------------------------------------------------------------------- 2: against enumeration
def _enumeration(name, p, Y):
    if name.startswith("bsc"):
        return E.enum_linear(Y, p["W"], p["sigma"], [0., 1.], np.log([1 - p["pi"], p["pi"]]), mu=p.get("mu"))
    if name in ("mca", "mmca"):
        return E.enum_mca(Y, p["W"], 6.0 if name == "mmca" else 21.0, name == "mmca", p["pi"], p["sigma"])
    if name.startswith("dsc"):
        states = {"dsc3": [-1., 0., 1.], "dsc4": [0., 1., 2., 3.]}[name]
        return E.enum_linear(Y, p["W"], p["sigma"], states, np.log(p["pi"]))
    if name == "tsc":
        return E.enum_linear(Y, p["W"], p["sigma"], [-1., 0., 1.], np.log([p["pi"] / 2, 1 - p["pi"], p["pi"] / 2]))
    return E.enum_gsc(p, Y)


@pytest.mark.parametrize("name", sorted(ENUM_SHAPE))
def test_against_enumeration(dev, name):
    D, H, seed = ENUM_SHAPE[name]
    N = 300
    m, p, Y, _, _ = _problem(name, np.random.RandomState(seed), D, H, N, H, H)
    want = _enumeration(name, p, Y)
    got = m.encode(p, {"y": Y})
    keep = np.ones(N, dtype=bool)
    if name == "tsc":              # rows whose candidates repeat a latent hold pseudo-states: not the model's posterior
        keep = _tsc_distinct(p, Y, D, H)
        assert keep.sum() >= N // 2, keep.sum()
    _check(name, [g[keep] for g in got], [w[keep] for w in want])
    _in_range(got, name in BINARY)


# ---------------------------------------------------------------------------------- 3: consistency with reconstruct()
@pytest.mark.parametrize("name,D,H,Hp,g", [("bsc", 25, 10, 8, 5), ("bsc_mu", 64, 40, 8, 4), ("dsc3", 25, 10, 7, 5),
                                           ("dsc4", 64, 32, 6, 3), ("tsc", 12, 6, 6, 6), ("gsc_scalar", 25, 10, 7, 4),
                                           ("gsc_full", 40, 16, 5, 3)])
def test_mean_reproduces_reconstruct(dev, name, D, H, Hp, g):
    N = 300 if name == "tsc" else 160
    m, p, Y, _, _ = _problem(name, np.random.RandomState(1 if name == "tsc" else D + H), D, H, N, Hp, g)
    mean, _ = m.encode(p, {"y": Y})
    want = m.reconstruct(p, {"y": Y})
    got = mean @ np.asarray(p["W"]).T + (0.0 if p.get("mu") is None or name.startswith("gsc") else p["mu"][None, :])
    keep = np.ones(N, dtype=bool)
    if name == "tsc":              # the rows with distinct candidates
        keep = _tsc_distinct(p, Y, D, H)
        assert keep.sum() >= N // 2, keep.sum()
    err = R.row_rel_err(got[keep], want[keep])
    print("encode %-30s mean W^T + mu against reconstruct(): %.3e (bound %.1e)" % (name, err, RTOL))
    assert err <= RTOL


# -------------------------------------------------------------------------------------------------------- 4: exact=True
@pytest.mark.parametrize("name,D,H", [("bsc", 20, 6), ("bsc_mu", 20, 6), ("bsc", 20, 13), ("mca", 20, 6), ("mmca", 20, 6),
                                      ("mca", 70, 10), ("mmca", 70, 10)])
def test_exact_against_enumeration(dev, name, D, H):
    N = 37 if H < 13 else 20
    m, p, Y, _, _ = _problem(name, np.random.RandomState(7 * D + H), D, H, N, min(H, 3), 2)
    p_in = _copy(p)
    calls = _entries(m)
    got = m.encode(p, {"y": Y}, exact=True)
    for k in p_in:
        np.testing.assert_array_equal(p[k], p_in[k])
    assert ("pm_encode_exact_mca_f64" if name in ("mca", "mmca") else "pm_recon_exact_lin_f64") in calls, calls
    assert not [c for c in calls if "estep" in c or "select" in c or c == "pm_encode_f64"], calls
    _check("exact %s D=%d H=%d" % (name, D, H), got, _enumeration(name, p, Y))
    _in_range(got, True)


@pytest.mark.parametrize("name,D,H", [("bsc", 20, 10), ("mca", 20, 10), ("mmca", 20, 10)])
def test_exact_against_the_truncated_path_at_full_width(dev, name, D, H):
    N = 100
    small, p, Y, _, _ = _problem(name, np.random.RandomState(50 + H + len(name)), D, H, N, 3, 2)
    full = _problem(name, np.random.RandomState(0), D, H, 1, H, H)[0]
    got = small.encode(p, {"y": Y}, exact=True)
    _check("exact %s H=%d against H'=gamma=H" % (name, H), got, full.encode(p, {"y": Y}), rtol=2e-11)


# ------------------------------------------------------------------------------------------------ 5: masks and weights
def _observed(rng, N, D, frac=0.5):
    M = rng.uniform(size=(N, D)) < frac
    for n in range(N):                                   # at least two observed dimensions per row
        while M[n].sum() < 2:
            M[n, rng.randint(D)] = True
    return M


def _masked_enumeration(name, p, Y, M):
    out = [np.empty((Y.shape[0], p["W"].shape[1])) for _ in range(2)]
    for n in range(Y.shape[0]):
        o = np.nonzero(M[n])[0]
        q = dict(p, W=p["W"][o])
        if p.get("mu") is not None:
            q["mu"] = p["mu"][o]
        mean, prob = _enumeration(name, q, Y[n:n + 1, o])
        out[0][n], out[1][n] = mean[0], prob[0]
    return out


@pytest.mark.parametrize("name", ["bsc", "bsc_mu", "mca", "mmca"])
def test_masks_and_weights(dev, name):
    D, H, N = 12, 6, 60
    rng = np.random.RandomState(200 + len(name))
    m, p, Y, _, _ = _problem(name, rng, D, H, N, H, H)
    if name in ("mca", "mmca"):
        p = m.check_params(_copy(p))
    plain = m.encode(p, {"y": Y})
    calls = _entries(m)
    ones = m.encode(p, {"y": Y, "mask": np.ones((N, D), dtype=bool)})
    assert "pm_encode_f64" in calls, calls
    _check("%s all-ones mask against the unmasked call" % name, ones, plain)
    M = _observed(rng, N, D)
    masked = m.encode(p, {"y": Y, "mask": M})
    _check("%s 50%% observed against enumeration" % name, masked, _masked_enumeration(name, p, Y, M))
    _in_range(masked, True)
    _bits(m.encode(p, {"y": Y, "weight": M.astype(np.float64)}), masked, "a {0, 1} weight gives the masked call's bits")
    for hole in (np.nan, np.inf, -np.inf, 1e300):
        Yh = np.where(M, Y, hole)
        _bits(m.encode(p, {"y": Yh, "mask": M}), masked, "mask: %r in the holes" % hole)
        _bits(m.encode(p, {"y": Yh, "weight": M.astype(np.float64)}), masked, "weight: %r in the holes" % hole)


# ------------------------------------------------------------------------------------------------------------ 6: bits
@pytest.mark.parametrize("name", ["bsc_mu", "mca", "mmca", "dsc4", "tsc", "gsc_scalar", "gsc_full", "mog_diagonal", "mog_full",
                                  "mop_A"])
def test_bits_repeat_across_calls_models_builds_row_order_shards_and_device_output(dev, name):
    import torch
    from prosper_amd.em.camodels._device import DeviceArray
    rng = np.random.RandomState(13)
    if name.startswith("mo"):
        mk = lambda: _mixture(name, np.random.RandomState(13), 24, 9, 700)
        m, p, Y, _ = mk()
        fresh = mk()[0]
    else:
        m, p, Y, _, _ = _problem(name, rng, 24, 12, 700, 5, 3)
        fresh = _problem(name, np.random.RandomState(0), 24, 12, 1, 5, 3)[0]
    a = m.encode(p, {"y": Y})
    _bits(m.encode(p, {"y": Y}), a, "second call")
    _bits(fresh.encode(p, {"y": Y}), a, "fresh model")
    d = m.encode(p, {"y": Y}, device=True)
    assert all(isinstance(t, DeviceArray) and t.tensor.is_cuda and t.tensor.is_contiguous() for t in d)
    _bits(d, a, "device=True")
    if hasattr(m, "deterministic") and name != "gsc_full":      # (GSC's deterministic mode is built for a scalar sigma_sq)
        m.deterministic = True
        _bits(m.encode(p, {"y": Y}), a, "deterministic library")
        m.deterministic = False
    perm = rng.permutation(len(Y))
    _bits(m.encode(p, {"y": Y[perm]}), [t[perm] for t in a], "row permutation")
    _bits(m.encode(p, {"y": Y[123:389]}), [t[123:389] for t in a], "shard")
    _bits(m.encode(p, {"y": torch.from_numpy(Y).to(dev)}), a, "device input")


@pytest.mark.parametrize("name", ["bsc", "mca", "mmca", "dsc3", "tsc", "gsc_full", "mog_diagonal", "mog_full", "mop"])
def test_nan_row_and_empty(dev, name):
    rng = np.random.RandomState(11)
    if name.startswith("mo"):
        m, p, Y, _ = _mixture(name, rng, 6, 5, 70)
    else:
        m, p, Y, _, _ = _problem(name, rng, 6, 5, 70, 3, 2)
    clean_rows = m.encode(p, {"y": np.delete(Y, 13, axis=0)})
    Y = Y.copy()
    Y[13, 2] = np.nan
    rows = m.encode(p, {"y": Y})
    for t, c in zip(rows, clean_rows):
        assert np.isnan(t[13]).all() and np.isfinite(np.delete(t, 13, axis=0)).all()
        np.testing.assert_array_equal(np.delete(t, 13, axis=0), c)
    calls = _entries(m) if hasattr(m, "_call") else []
    empty = m.encode(p, {"y": np.zeros((0, 6))})
    assert all(t.shape == (0, 5) and t.dtype == np.float64 for t in empty) and not calls
    assert all(t.shape == (0, 5) for t in m.encode(p, {"y": np.zeros((0, 6))}, device=True))


# ------------------------------------------------------------------------------------------- 7: training undisturbed
def _train(m, params, Y, Yh, steps, interleave):
    a = _schedule(steps)
    for _ in range(steps):
        params = m.step(a, params, {"y": Y})
        if interleave:
            hp = (getattr(m, "Hprime", None), getattr(m, "gamma", None))
            mean, prob = m.encode(_copy(params), {"y": Yh})
            assert mean.shape == prob.shape == (len(Yh), m.H) and np.isfinite(mean).all() and np.isfinite(prob).all()
            assert (getattr(m, "Hprime", None), getattr(m, "gamma", None)) == hp
        a.next()
    return _copy(params), getattr(m, "spec_hits", None)


@pytest.mark.parametrize("name", ["bsc", "mca", "mmca", "dsc3", "tsc", "gsc_scalar", "mog_diagonal", "mog_full", "mop"])
def test_training_undisturbed(dev, name):
    rng = np.random.RandomState(14)
    N, Nh = 1500, 300
    if name.startswith("mo"):
        D, H = 12, 5
        _, p, Y, _ = _mixture(name, rng, D, H, N + Nh)
        mk = lambda: _mixture(name, np.random.RandomState(0), D, H, 4)[0]
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
    ref, hits_ref = _train(det(), _copy(p), Yt, Yh, 6, False)
    got, hits_got = _train(det(), _copy(p), Yt, Yh, 6, True)
    for k in ref:
        np.testing.assert_array_equal(ref[k], got[k], err_msg=k)
    if name in ("bsc", "gsc_scalar"):
        assert hits_ref is not None and hits_ref == hits_got, (hits_ref, hits_got)


# ---------------------------------------------------------------------------------------------------------- 8: limits
def test_limits_raise_hip_error(dev):
    from prosper_amd import _lib
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    rng = np.random.RandomState(6)
    D, N = 16, 12
    Y = rng.normal(size=(N, D))
    with pytest.raises(_lib.HipError):                   # H' = 17 > PM_MAX_HPRIME
        BSC_ET(D, 40, 17, 2).encode({"W": rng.normal(size=(D, 40)), "pi": 0.05, "sigma": 1.0}, {"y": Y})
    with pytest.raises(_lib.HipError):                   # exact: 2^33 states
        BSC_ET(D, 33, 3, 2).encode({"W": rng.normal(size=(D, 33)), "pi": 0.05, "sigma": 1.0}, {"y": Y}, exact=True)
    with pytest.raises(_lib.HipError):
        MCA_ET(D, 33, 3, 2).encode({"W": rng.uniform(0.5, 2, size=(D, 33)), "pi": 0.05, "sigma": 1.0},
                                   {"y": np.abs(Y)}, exact=True)
    D = 1025
    with pytest.raises(_lib.HipError):                   # exact, MCA: D > 1024
        MCA_ET(D, 8, 4, 2).encode({"W": rng.uniform(0.5, 2, size=(D, 8)), "pi": 0.2, "sigma": 1.0},
                                  {"y": rng.uniform(0, 2, size=(5, D))}, exact=True)
