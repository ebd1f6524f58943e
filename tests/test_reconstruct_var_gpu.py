"""reconstruct(variance=True) on the device: the posterior variance V of the noiseless value against NumPy
enumeration of every state at H' = gamma = H, against the E-step's own log-joints on truncated state sets (one case per branch
of the kernels of recon_var.hip), with masks, bit for bit repeatable, with a training run undisturbed, at the edges and
limits, and through reconstruct_image().  NumPy references: tests/recon_var_reference.py (pinned on the CPU by
tests/test_reconstruct_var_cpu.py); problems and mixtures: tests/test_reconstruct_gpu.py, masks: tests/test_masked_gpu.py.

Tolerance, per row: max_d |V - V_ref| <= 4e-11 max_d E_ref[ybar_d^2] (RV.VTOL).  It follows from the project's 1e-11
row-relative on yhat: yhat^2 carries 2e-11 of max yhat^2 <= max E[ybar^2], the second moment runs through the same expectation
and product pipeline for another 1e-11, the rest is margin.  ``Yhat`` must have the bits of the call without the keyword.  The
deviations measured on the MI355X are recorded in DESIGN 4.19."""
import numpy as np
import pytest

import recon_reference as R
import recon_var_reference as RV
from test_masked_gpu import _capture, _mask
from test_masked_gpu import _problem as _masked_problem
from test_reconstruct_gpu import ENUM, ENUM_SHAPE, _gsc_params, _mixture, _problem, _schedule, _tsc_distinct

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _bits(a, b, what=""):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), what


def _check(tag, got, ref, keep=None):
    V = got if keep is None else got[keep]
    ref = ref if keep is None else RV.Moments(*(x[keep] for x in ref))
    err = RV.row_err(V, ref)
    print("reconstruct variance %-30s max_d |V - V_ref| / max_d E[ybar^2] %.3e (bound %.1e)" % (tag, err, RV.VTOL))
    assert V.shape == ref.V.shape and V.dtype == np.float64
    assert (V >= 0).all(), tag
    assert err <= RV.VTOL, (tag, err)


def _both(m, p, data, **kw):
    """(Yhat, V) of the call with the keyword, Yhat checked bit for bit against the call without it."""
    plain = m.reconstruct(p, dict(data), **kw)
    out = m.reconstruct(p, dict(data), variance=True, **kw)
    assert isinstance(out, tuple) and len(out) == 2
    _bits(np.asarray(out[0]), np.asarray(plain), "Yhat changed with variance=True")
    return np.asarray(out[0]), np.asarray(out[1])


def _entries(m):
    calls = []
    orig = m._call
    m._call = lambda label, entry, *args: (calls.append(entry), orig(label, entry, *args))[1]
    return calls


# ------------------------------------------------------------------------------------------- 1: against full enumeration
def _enum_ref(name, p, Y, m):
    if name in ("bsc", "bsc_mu"):
        return RV.enum_linear(Y, p["W"], p["sigma"], [0., 1.], np.log([1 - p["pi"], p["pi"]]), mu=p.get("mu"))
    if name in ("mca", "mmca"):
        return RV.enum_mca(Y, p["W"], 6.0 if name == "mmca" else 21.0, name == "mmca", p["pi"], p["sigma"])
    if name.startswith("dsc"):
        return RV.enum_linear(Y, p["W"], p["sigma"], m.states, np.log(p["pi"]))
    if name == "tsc":
        return RV.enum_linear(Y, p["W"], p["sigma"], [-1., 0., 1.], np.log([p["pi"] / 2, 1 - p["pi"], p["pi"] / 2]))
    return RV.enum_gsc(p, Y)


@pytest.mark.parametrize("name", ENUM)
def test_against_enumeration(dev, name):
    D, H, seed = ENUM_SHAPE[name]
    N = 300
    m, p, Y, clean, _ = _problem(name, np.random.RandomState(seed), D, H, N, H, H)
    p_in = {k: np.array(v, copy=True) for k, v in p.items()}
    ref = _enum_ref(name, p, Y, m)
    yhat, V = _both(m, p, {"y": Y})
    for k in p_in:
        np.testing.assert_array_equal(p[k], p_in[k])
    assert set(p) == set(p_in) and (m.Hprime, m.gamma) == (H, H)
    keep = np.ones(N, dtype=bool)
    if name == "tsc":              # rows whose candidates repeat a latent hold pseudo-states: not the model's posterior
        keep = _tsc_distinct(p, Y, D, H)
        assert keep.sum() >= N // 2
    assert R.row_rel_err(yhat[keep], ref.yhat[keep]) <= 1e-11
    _check(name, V, ref, keep)
    print("reconstruct variance %-30s sum (yhat - clean)^2 / sum V = %.4f" % (name, RV.calibration(yhat[keep], V[keep],
                                                                                                  clean[keep])))


@pytest.mark.parametrize("kind", ["mog_diagonal", "mog_full", "mop", "mop_A"])
def test_mixtures_against_numpy(dev, kind):
    m, p, Y, want = _mixture(kind, np.random.RandomState(31 + len(kind)), 10, 6, 250)
    if kind.startswith("mop"):
        ref = RV.mop(m.normalize(Y) if kind == "mop_A" else Y, p["W"], p["pies"])
    else:
        ref = RV.mog(Y, p["W"], p["pies"], p["sigmas_sq"])
    assert R.row_rel_err(ref.yhat, want) < 1e-12
    yhat, V = _both(m, p, {"y": Y})
    _check(kind, V, ref)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_bsc_calibration_at_the_exact_posterior(dev, seed):
    """Data drawn from the model, exact posterior (H' = gamma = H): sum (yhat - ybar_clean)^2 / sum V in [0.95, 1.05], the
    condition tests/test_reconstruct_var_cpu.py holds the NumPy reference to at the same settings."""
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    rng = np.random.RandomState(seed)
    D, H, N, pi, sigma = 16, 6, 4000, 0.3, 2.0
    W = rng.normal(size=(D, H))
    clean = (rng.uniform(size=(N, H)) < pi) @ W.T
    Y = clean + sigma * rng.normal(size=(N, D))
    yhat, V = _both(BSC_ET(D, H, H, H), {"W": W, "pi": pi, "sigma": sigma}, {"y": Y})
    _check("bsc calibration seed %d" % seed, V, RV.enum_linear(Y, W, sigma, [0., 1.], np.log([1 - pi, pi])))
    ratio = RV.calibration(yhat, V, clean)
    print("reconstruct variance calibration seed %d: %.4f" % (seed, ratio))
    assert 0.95 <= ratio <= 1.05


# ----------------------------------------------------------------- 2: against the E-step's own log-joints, truncated
def _truncated_reference(m, name, p, Y):
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
        assert (0.5 * lp).max(axis=1).min() > -650.0      # (no row whose weights all underflow: the DBL_MIN floor stays invisible)
        return RV.gsc_from_lpj(p, Y, lp, cand, m.state_matrix), cand
    lp, cand = m.compute_lpj(LoglikPoint(), dict(p), {"y": Y})
    lp, cand = np.asarray(lp), np.asarray(cand)
    if name in ("mca", "mmca"):
        return RV.mca_from_lpj(lp, cand, m.state_matrix, p["W"], m._rho(1.0), name == "mmca"), cand
    table = m.state_matrix if m.no_states else None
    if name.startswith("bsc"):
        return RV.linear_from_lpj(lp, 1.0, cand, p["W"], (1.0,), 1, 1 + H, table, mu=p.get("mu")), cand
    if name.startswith("dsc"):
        blocks = [v for v in m.states if v != 0.]
        return RV.linear_from_lpj(lp, 1.0, cand, p["W"], blocks, 1, 1 + len(blocks) * H, table), cand
    return RV.linear_from_lpj(lp, 1.0, cand, p["W"], (), 0, 0, m.state_matrix), cand


# (name, D, H, H', gamma) -> the branch of recon_var.hip it reaches
TRUNC = [
    ("bsc", 12, 10, 1, 1),          # H' = 1: no pairs, no table (p = NULL, finish without pairs)
    ("bsc_mu", 12, 10, 2, 2),       # H' = 2: one pair; mu
    ("bsc", 40, 48, 12, 2),         # 66 pairs: a lane owns two
    ("bsc", 40, 48, 16, 2),         # 120 pairs: PM_MAX_HPRIME
    ("bsc", 25, 12, 10, 4),         # S = 375 > 256: a second LDS chunk of table states
    ("dsc3", 20, 65, 4, 2),         # H = 65: one lane takes a second latent; 2 non-zero values
    ("dsc4", 24, 130, 12, 2),       # H = 130: three trips of the H loop
    ("dsc8", 16, 12, 3, 2),         # 7 non-zero values: nblk = 7
    ("tsc", 24, 70, 5, 3),          # H = 70 with table states only
    ("tsc", 12, 6, 6, 3),           # rows with a repeated candidate (asserted below): pseudo-states
    ("tsc", 25, 10, 7, 5),
    # finish kernel: D around a wavefront's 64 lanes (D = 1, where every latent's selection score |y| ties and the E-step
    # kernels may rank differently, runs through the C ABI: tests/test_reconstruct_var_abi_gpu.py)
    ("bsc_mu", 63, 10, 4, 2), ("bsc", 64, 10, 4, 2), ("bsc_mu", 65, 10, 4, 2),
    ("bsc", 1100, 10, 4, 2),        # ... past 1024, eighteen trips of a lane
    ("mca", 1, 8, 3, 2), ("mmca", 1, 8, 3, 2), ("mca", 70, 24, 6, 3), ("mmca", 70, 24, 6, 3),           # recon_mca_var_kernel<DPL>
    ("mca", 1024, 24, 6, 3), ("mmca", 1024, 24, 6, 3),
    ("mca", 25, 10, 8, 5), ("mmca", 25, 10, 7, 5),
    ("gsc_scalar", 25, 10, 7, 4), ("gsc_diagonal", 48, 24, 6, 3), ("gsc_full", 40, 16, 5, 3), ("gsc_scalar", 16, 70, 4, 2),
]


@pytest.mark.parametrize("name,D,H,Hp,g", TRUNC)
def test_against_the_esteps_log_joints(dev, name, D, H, Hp, g):
    N = 96 if D < 1000 else 40
    m, p, Y, _, _ = _problem(name, np.random.RandomState(D + H + Hp), D, H, N, Hp, g)
    if name in ("mca", "mmca"):
        p = m.check_params({k: np.array(v, copy=True) for k, v in p.items()})
    ref, cand = _truncated_reference(m, name, p, Y)
    if (name, H) == ("tsc", 6):
        assert sum(len(set(c)) < Hp for c in cand) >= 5, "too few rows with a repeated candidate"
    calls = _entries(m)
    yhat, V = _both(m, p, {"y": Y})
    want = {"pm_recon_gsc_moments2_f64" if name.startswith("gsc") else "pm_recon_moments2_f64", "pm_recon_var_finish_f64"}
    assert want <= set(calls) and ("pm_recon_mca_var_f64" in calls) == (name in ("mca", "mmca")), calls
    assert R.row_rel_err(yhat, ref.yhat) <= 1e-11
    _check("%s D=%d H=%d H'=%d g=%d" % (name, D, H, Hp, g), V, ref)


@pytest.mark.parametrize("name", ["bsc", "mca", "dsc3", "gsc_scalar", "mog_diagonal"])
def test_second_trip_of_the_row_loops(dev, name):
    """N = 8269 > 2048 workgroups of four rows: every wavefront of the first workgroups takes a second row in each kernel of
    recon_var.hip.  The rows from 100 before the boundary to the end against the NumPy sums over those rows alone; the whole
    result bit for bit against the same call on shards of 2048 rows."""
    D, H, Hp, g, N = 8, 6, 4, 2, 8269
    tail = slice(8192 - 100, N)
    if name.startswith("mo"):
        m, p, Y, _ = _mixture(name, np.random.RandomState(5), D, H, N)
        ref = RV.mog(Y[tail], p["W"], p["pies"], p["sigmas_sq"])
    else:
        m, p, Y, _, _ = _problem(name, np.random.RandomState(900 + len(name)), D, H, N, Hp, g)
        if name == "mca":
            p = m.check_params({k: np.array(v, copy=True) for k, v in p.items()})
        ref, _ = _truncated_reference(m, name, p, Y[tail])
    yhat, V = m.reconstruct(p, {"y": Y}, variance=True)
    assert V.shape == (N, D) and np.isfinite(V).all()
    _check("%s second trip" % name, V[tail], ref)
    shards = [m.reconstruct(p, {"y": Y[i:i + 2048]}, variance=True) for i in range(0, N, 2048)]
    _bits(np.concatenate([s[0] for s in shards]), yhat)
    _bits(np.concatenate([s[1] for s in shards]), V)


# ------------------------------------------------------------------------------------------------------------ 3: masks
@pytest.mark.parametrize("kind", ["bsc", "bsc_mu", "mca", "mmca"])
def test_masks_against_the_masked_log_joints(dev, kind):
    """50 % observed, row 0 fully observed, row 1 not at all: V against the NumPy sum over the masked E-step's own log-joints
    and candidates (all D dimensions: the variance given the observed pixels); whatever the holes hold, the same bits."""
    D, H, Hp, g, N = 20, 12, 5, 3, 60
    rng = np.random.RandomState(40 + len(kind))
    m, p, Y = _masked_problem(kind, rng, D, H, N, Hp, g)
    M = _mask(rng, N, D)
    kept = _capture(m)
    calls = _entries(m)
    yhat, V = _both(m, p, {"y": np.where(M, Y, 0.0), "mask": M})
    out = kept["out"]
    lp, cand, lay = out["logpj"].cpu().numpy(), out["cand"].cpu().numpy(), out["lay"]
    if kind.startswith("bsc"):
        ref = RV.linear_from_lpj(lp, 1.0, cand, np.asarray(lay["W"]), (1.0,), 1, 1 + H, m.state_matrix, mu=p.get("mu"))
    else:
        ref = RV.mca_from_lpj(lp, cand, m.state_matrix, np.asarray(lay["W"]), m._rho(1.0), kind == "mmca")
    assert "pm_recon_moments2_f64" in calls and ("pm_recon_mca_var_f64" in calls) == (not kind.startswith("bsc")), calls
    assert R.row_rel_err(yhat, ref.yhat) <= 1e-11
    _check("masked " + kind, V, ref)
    assert np.isfinite(V).all() and (V[1] > 0).any()
    for hole in (np.nan, np.inf, 1e300):
        y2, V2 = m.reconstruct(p, {"y": np.where(M, Y, hole), "mask": M}, variance=True)
        _bits(y2, yhat, "hole %r" % hole)
        _bits(V2, V, "hole %r" % hole)


# ------------------------------------------------------------------------------------------------------------- 4: bits
@pytest.mark.parametrize("name", ["bsc_mu", "mca", "mmca", "dsc4", "tsc", "gsc_scalar", "gsc_full", "mog_diagonal", "mog_full",
                                  "mop_A"])
def test_bits_repeat_across_calls_builds_row_order_shards_and_device_output(dev, name):
    import torch
    from prosper_amd.em.camodels._device import DeviceArray
    rng = np.random.RandomState(13)
    if name.startswith("mo"):
        m, p, Y, _ = _mixture(name, rng, 24, 9, 700)
    else:
        m, p, Y, _, _ = _problem(name, rng, 24, 12, 700, 5, 3)
    yhat, V = _both(m, p, {"y": Y})
    _bits(m.reconstruct(p, {"y": Y}, variance=True)[1], V)
    d = m.reconstruct(p, {"y": Y}, device=True, variance=True)
    assert isinstance(d, tuple) and all(isinstance(t, DeviceArray) and t.tensor.is_cuda for t in d)
    _bits(np.asarray(d[0]), yhat)
    _bits(np.asarray(d[1]), V)
    if hasattr(m, "deterministic") and name != "gsc_full":      # (GSC's deterministic mode is built for a scalar sigma_sq)
        m.deterministic = True
        _bits(m.reconstruct(p, {"y": Y}, variance=True)[1], V, "deterministic library")
        m.deterministic = False
    perm = rng.permutation(len(Y))
    _bits(m.reconstruct(p, {"y": Y[perm]}, variance=True)[1], V[perm], "row permutation")
    _bits(m.reconstruct(p, {"y": Y[100:333]}, variance=True)[1], V[100:333], "shard")
    _bits(m.reconstruct(p, {"y": DeviceArray(torch.from_numpy(Y).to(dev))}, variance=True)[1], V)


@pytest.mark.parametrize("center", [False, True])
def test_reconstruct_image_variance(dev, center):
    """(image, var_map): the same two images for three values of ``chunk``, the image that of the call without the keyword,
    var_map the overlap average of the patches' V (``center=True`` adds the patch means to the estimates only)."""
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.utils import patches as U
    rng = np.random.RandomState(3)
    D, H = 16, 8
    m = BSC_ET(D, H, 4, 2)
    p = {"W": rng.normal(size=(D, H)), "pi": 0.25, "sigma": 0.8}
    img = rng.normal(size=(13, 15))
    plain = m.reconstruct_image(p, img, center=center)
    out = [m.reconstruct_image(p, img, center=center, chunk=c, variance=True) for c in (None, 7, 40)]
    for im, vm in out:
        assert im.shape == img.shape and vm.shape == img.shape and (vm >= 0).all() and vm.max() > 0
        _bits(im, plain)
        _bits(vm, out[0][1])
    Yp, means = U.extract_patches(img, 4, center=center)
    _, V = m.reconstruct(p, {"y": Yp}, variance=True)
    _bits(U.average_patches(V, img.shape, 4), out[0][1])
    d = U.denoise_image(m, p, img, center=center, variance=True, device=True)
    _bits(np.asarray(d[1]), out[0][1])


# ------------------------------------------------------------------------------------------- 5: training undisturbed
def _train(m, params, Y, Yh, steps, interleave):
    a = _schedule(steps)
    for _ in range(steps):
        params = m.step(a, params, {"y": Y})
        if interleave:
            hp = (getattr(m, "Hprime", None), getattr(m, "gamma", None))
            yh, V = m.reconstruct({k: np.array(v, copy=True) for k, v in params.items()}, {"y": Yh}, variance=True)
            assert V.shape == Yh.shape and np.isfinite(V).all() and (V >= 0).all() and np.isfinite(yh).all()
            assert (getattr(m, "Hprime", None), getattr(m, "gamma", None)) == hp
        a.next()
    return {k: np.array(v, copy=True) for k, v in params.items()}, getattr(m, "spec_hits", None)


@pytest.mark.parametrize("name", ["bsc", "mca", "dsc3", "tsc", "gsc_scalar", "mog_full", "mop"])
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
    ref, hits_ref = _train(det(), {k: np.array(v, copy=True) for k, v in p.items()}, Yt, Yh, 6, False)
    got, hits_got = _train(det(), {k: np.array(v, copy=True) for k, v in p.items()}, Yt, Yh, 6, True)
    for k in ref:
        np.testing.assert_array_equal(ref[k], got[k], err_msg=k)
    if name in ("bsc", "gsc_scalar"):
        assert hits_ref is not None and hits_ref == hits_got, (hits_ref, hits_got)


# ------------------------------------------------------------------------------------------------------------ 6: edges
@pytest.mark.parametrize("name", ["bsc", "mca", "mmca", "dsc3", "tsc", "gsc_full", "mog_diagonal", "mog_full", "mop"])
def test_nan_row_and_empty(dev, name):
    rng = np.random.RandomState(11)
    if name.startswith("mo"):
        m, p, Y, _ = _mixture(name, rng, 6, 5, 70)
    else:
        m, p, Y, _, _ = _problem(name, rng, 6, 5, 70, 3, 2)
    clean_rows = m.reconstruct(p, {"y": np.delete(Y, 13, axis=0)}, variance=True)[1]
    Y = Y.copy()
    Y[13, 2] = np.nan
    V = m.reconstruct(p, {"y": Y}, variance=True)[1]
    assert np.isnan(V[13]).all() and np.isfinite(np.delete(V, 13, axis=0)).all()
    _bits(np.delete(V, 13, axis=0), clean_rows)
    assert (np.delete(V, 13, axis=0) >= 0).all()
    calls = _entries(m) if hasattr(m, "_call") else []
    empty = m.reconstruct(p, {"y": np.zeros((0, 6))}, variance=True)
    assert all(e.shape == (0, 6) and e.dtype == np.float64 for e in empty) and not calls
    assert all(e.shape == (0, 6) for e in m.reconstruct(p, {"y": np.zeros((0, 6))}, device=True, variance=True))


@pytest.mark.parametrize("pi", [0.0, 1.0])
def test_bsc_prior_at_zero_and_one(dev, pi):
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    rng = np.random.RandomState(8)
    D, H, N = 6, 5, 40
    p = {"W": rng.normal(size=(D, H)), "pi": pi, "sigma": 0.9}
    Y = rng.normal(size=(N, D))
    if pi == 0.0:          # the null state alone carries weight: no spread
        yhat, V = BSC_ET(D, H, H, H).reconstruct(p, {"y": Y}, variance=True)
        np.testing.assert_array_equal(yhat, np.zeros((N, D)))
        np.testing.assert_array_equal(V, np.zeros((N, D)))
    else:                  # as reconstruct(): the E-step has no log-joints at pi = 1, the call raises as it does
        with pytest.raises(ZeroDivisionError):
            BSC_ET(D, H, H, H).reconstruct(p, {"y": Y}, variance=True)


def test_dsc_value_of_zero_prior(dev):
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    rng = np.random.RandomState(9)
    D, H, N = 6, 4, 50
    states = np.array([0., 1., 2., 3.])
    pi = np.array([0.6, 0.25, 0.0, 0.15])
    W, sigma = rng.normal(size=(D, H)), 0.8
    Y = rng.normal(size=(N, D)) * 2
    m = DSC_ET(D, H, H, H, states=states)
    yhat, V = _both(m, {"W": W, "pi": pi, "sigma": sigma}, {"y": Y})
    assert np.isfinite(V).all()
    with np.errstate(divide="ignore"):
        _check("dsc pi_k=0", V, RV.enum_linear(Y, W, sigma, states, np.log(pi)))


def test_indefinite_covariances_give_nan_rows(dev):
    from prosper_amd.em.camodels.gsc_et import GSC
    from prosper_amd.em.mixturemodels.MoG import MoG
    rng = np.random.RandomState(12)
    D, H = 5, 4
    p = _gsc_params(rng, D, H, "full")
    p["sigma_sq"] = np.diag([1., 1., -0.5, 1., 1.])
    out = GSC(D, H, 2, 2, sigma_sq_type="full").reconstruct(p, {"y": rng.normal(size=(9, D))}, variance=True)
    assert all(o.shape == (9, D) and np.isnan(o).all() for o in out)
    sig = np.stack([np.eye(D)] * H)
    sig[2] = np.diag([1., -1., 1., 1., 1.])
    q = {"W": rng.normal(size=(D, H)), "pies": np.full(H, 1.0 / H), "sigmas_sq": sig}
    out = MoG(D, H, sigmas_sq_type="full").reconstruct(q, {"y": rng.normal(size=(9, D))}, variance=True)
    assert all(o.shape == (9, D) and np.isnan(o).all() for o in out)


# ---------------------------------------------------------------------------------------------- 7: limits and refusals
def test_limits_and_refusals_come_before_any_launch(dev):
    from prosper_amd import _lib
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    rng = np.random.RandomState(5)
    D, H, N = 16, 12, 20
    Y = rng.normal(size=(N, D))
    p = {"W": rng.normal(size=(D, H)), "pi": 0.2, "sigma": 1.0}
    m = BSC_ET(D, H, 4, 2)
    calls = _entries(m)
    with pytest.raises(NotImplementedError, match="variance"):
        m.reconstruct(p, {"y": Y}, exact=True, variance=True)
    with pytest.raises(NotImplementedError, match="exact=True with a mask"):
        m.reconstruct(p, {"y": Y, "mask": np.ones((N, D), dtype=bool)}, exact=True, variance=True)
    assert not calls
    d = DSC_ET(D, H, 4, 2)
    calls = _entries(d)
    with pytest.raises(NotImplementedError, match="DSC_ET.*mask"):
        d.reconstruct({"W": p["W"], "pi": np.array([0.8, 0.2]), "sigma": 1.0}, {"y": Y, "mask": np.ones((N, D), dtype=bool)},
                      variance=True)
    assert not calls
    b17 = BSC_ET(D, 40, 17, 2)                   # (the constructor takes H' = 17: the refusal is reconstruct's)
    calls = _entries(b17)
    with pytest.raises(_lib.HipError, match="variance=True holds H' <= 16"):
        b17.reconstruct({"W": rng.normal(size=(D, 40)), "pi": 0.05, "sigma": 1.0}, {"y": Y}, variance=True)
    assert not calls
    q = {"W": rng.uniform(0.5, 2.0, size=(1025, 8)), "pi": 0.2, "sigma": 1.0}
    mca = MCA_ET(1025, 8, 4, 2)
    calls = _entries(mca)
    with pytest.raises(_lib.HipError, match="variance=True holds D <= 1024"):
        mca.reconstruct(q, {"y": rng.uniform(0, 2, size=(5, 1025))}, variance=True)
    assert not calls
