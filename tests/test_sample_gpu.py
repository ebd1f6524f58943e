"""sample_posterior() on the device: the drawn states, latent values and decoded rows against
tests/sample_reference.py on the E-step's own log-joints, the bit guarantees (a second call, the deterministic library, a row
permutation, a shard, a forced small chunk, the content of unobserved entries), the statistical tie to reconstruct() and
reconstruct(variance=True), the seeded path, the refusals, the second trip of the row loops and two ranks.

Tolerances.  Indices and the discrete models' latent values are exact (the uniforms are first moved off the reference's CDF
edges: tests/test_sample_abi_gpu.py).  Decoded rows: the project's 1e-11 row-relative bound of tests/test_reconstruct_gpu.py,
for GSC too (that file holds GSC to the same bound).  The statistical tie: the mean of M independent draws of a pixel has
standard deviation sqrt(V / M); six of them is passed by a correct sampler on one of ~200 pixels with probability < 200 * 2e-9
(Gaussian tail; the Berry-Esseen correction at M = 4096 is of the same order for these bounded or Gaussian-mixture draws)."""
import numpy as np
import pytest

import recon_reference as R
import sample_reference as SR
import test_reconstruct_gpu as TR

pytestmark = pytest.mark.gpu

RTOL = 1e-11


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _make(name, rng, D, H, N, Hp, g):
    """(model, params, Y): the problems of tests/test_reconstruct_gpu.py."""
    if name.startswith("mo"):
        m, p, Y, _ = TR._mixture(name, rng, D, H, N)
        return m, p, Y
    m, p, Y, _, _ = TR._problem(name, rng, D, H, N, Hp, g)
    if name in ("mca", "mmca"):
        p = m.check_params({k: np.array(v, copy=True) for k, v in p.items()})
    return m, p, Y


def _layout(m, name, p, Y):
    """What the reference needs of the model's E-step: dict(lp, cand, kw of SR.weights, draw(idx, E) -> (Ys, S))."""
    from prosper_amd.em.camodels._device import LoglikPoint
    H = m.H
    if name.startswith("mo"):
        W = np.asarray(p["W"])
        if name.startswith("mop"):
            X = m.normalize(Y) if name == "mop_A" else Y
            with np.errstate(divide="ignore"):
                lp = X @ np.log(W) - W.sum(0)[None, :] + np.log(p["pies"])[None, :]
        else:
            sig = p["sigmas_sq"]
            lp = np.empty((len(Y), H))
            for h in range(H):
                r = Y - W[:, h][None, :]
                if sig.ndim == 2:
                    lp[:, h] = -0.5 * (r * r / sig[h]).sum(1) - 0.5 * np.log(sig[h]).sum()
                else:
                    lp[:, h] = -0.5 * (r * np.linalg.solve(sig[h], r.T).T).sum(1) - 0.5 * np.linalg.slogdet(sig[h])[1]
            lp = lp + np.log(p["pies"])[None, :]

        def draw(idx, E=None):
            ai, av = SR.active_list(idx, None, H, (1.0,), 0, 0, None, 1)
            return SR.decode_linear(ai, av, W), SR.latents_from_active(ai, av, H)
        return dict(lp=lp, kw={}, draw=draw)
    if name.startswith("gsc"):
        saved = m._eval_begin()
        try:
            m._lpi_scale = 2.0
            lp, cand = m.compute_lpj(None, dict(p), {"y": Y})
            lp, cand = np.asarray(lp), np.asarray(cand)
        finally:
            m._eval_end(saved)
        SM, g = m.state_matrix, int(m.gamma)

        def draw(idx, E):
            ai, av = SR.gsc_active_list(idx, cand, SM, p, Y, E, max(g, 1))
            return SR.decode_linear(ai, av, np.asarray(p["W"])), SR.latents_from_active(ai, av, H)
        return dict(lp=lp, kw=dict(SR.GSC_WEIGHTS, lse=np.zeros(len(Y))), draw=draw)
    lp, cand = m.compute_lpj(LoglikPoint(), dict(p), {"y": Y})
    lp, cand = np.asarray(lp), np.asarray(cand)
    SM = np.asarray(m.state_matrix, dtype=np.float64)
    if name in ("mca", "mmca"):
        def draw(idx, E=None):
            A = max(1, int(SM.sum(1).max())) if len(SM) else 1
            ai, av = SR.active_list(idx, cand, H, (1.0,), 1, 1 + H, SM if len(SM) else None, A)
            return (SR.decode_mca(idx, cand, SM, np.asarray(p["W"]), m._rho(1.0), name == "mmca"),
                    SR.latents_from_active(ai, av, H))
        return dict(lp=lp, kw={}, draw=draw)
    if name.startswith("bsc"):
        blocks, soff, moff = (1.0,), 1, 1 + H
    elif name.startswith("dsc"):
        blocks = tuple(float(v) for v in m.states if v != 0.)
        soff, moff = 1, 1 + len(blocks) * H
    else:
        blocks, soff, moff = (), 0, 0
    table = SM if len(SM) else None

    def draw(idx, E=None):
        A = max(1, int((SM != 0).sum(1).max())) if len(SM) else 1
        ai, av = SR.active_list(idx, cand, H, blocks, soff, moff, table, A)
        return SR.decode_linear(ai, av, np.asarray(p["W"]), p.get("mu")), SR.latents_from_active(ai, av, H)
    return dict(lp=lp, kw={}, draw=draw)


def _rel(got, want):
    M, N, D = want.shape
    return R.row_rel_err(got.reshape(M * N, D), want.reshape(M * N, D))


def _normals(m, name, rng, N, M):
    return {"normals": rng.normal(size=(N, M, int(m.gamma)))} if name.startswith("gsc") else {}


# (name, D, H, H', gamma, M): K within 64 columns, over several chunks with a ragged last one, S = 0 (H' = 1), M = 1 / 64 / 65,
# D = 1 / 64 / 65 / 1024 for both decode kernels, H' = 16, GSC at gamma = 2, 3, 4, 6, 8 (H' = gamma), DSC with 8 values, TSC
# with latents held twice, every mixture kind
CASES = [("bsc", 25, 10, 8, 5, 1), ("bsc_mu", 64, 24, 6, 3, 64), ("bsc", 65, 130, 12, 3, 65), ("bsc", 40, 48, 16, 2, 3),
         ("bsc_mu", 1, 9, 1, 1, 5), ("bsc", 1024, 12, 4, 2, 2),
         ("mca", 1, 10, 4, 2, 3), ("mca", 64, 24, 6, 3, 64), ("mmca", 65, 24, 6, 3, 65), ("mmca", 1024, 12, 5, 2, 2),
         ("mca", 12, 8, 1, 1, 4), ("mca", 30, 40, 16, 2, 2),
         ("dsc4", 24, 130, 12, 3, 4), ("dsc8", 16, 12, 3, 2, 7), ("tsc", 24, 70, 5, 3, 6),
         ("gsc_scalar", 20, 12, 2, 2, 5), ("gsc_scalar", 20, 12, 3, 3, 64), ("gsc_diagonal", 20, 12, 4, 4, 3),
         ("gsc_full", 16, 12, 6, 6, 2), ("gsc_scalar", 18, 12, 8, 8, 2),
         ("mog_diagonal", 10, 6, 0, 0, 65), ("mog_full", 40, 21, 0, 0, 3), ("mop", 65, 70, 0, 0, 4), ("mop_A", 10, 6, 0, 0, 1)]


@pytest.mark.parametrize("name,D,H,Hp,g,M", CASES)
def test_draws_against_the_reference(dev, name, D, H, Hp, g, M):
    rng = np.random.RandomState(D + H + Hp + M)
    N = 24
    m, p, Y = _make(name, rng, D, H, N, Hp, g)
    p_in = {k: np.array(v, copy=True) for k, v in p.items()}
    lay = _layout(m, name, p, Y)
    U, moved = SR.nudge(rng.uniform(size=(N, M)), SR.cdfs(lay["lp"], **lay["kw"]))
    kw = _normals(m, name, rng, N, M)
    calls = TR._entries(m) if hasattr(m, "_call") else None
    Ys, S = m.sample_posterior(p, {"y": Y}, n_samples=M, uniforms=U, latents=True, **kw)
    assert Ys.shape == (M, N, D) and Ys.dtype == np.float64 and S.shape == (M, N, H) and S.dtype == np.float64
    for k in p_in:
        np.testing.assert_array_equal(p[k], p_in[k])
    if calls is not None:
        assert "pm_sample_states_f64" in calls, calls
        assert ("pm_sample_decode_mca_f64" in calls) == (name in ("mca", "mmca")), calls
        assert ("pm_sample_gsc_f64" in calls) == name.startswith("gsc"), calls
        assert ("pm_sample_decode_lin_f64" in calls) == (name not in ("mca", "mmca")), calls
    idx = SR.draw_states(lay["lp"], U, **lay["kw"])
    assert (idx >= 0).all()
    want, S_want = lay["draw"](idx, kw.get("normals"))
    err = _rel(Ys, want)
    print("sample_posterior %-12s D=%d H=%d H'=%d g=%d M=%d K=%d: row-relative error %.3e (%d uniforms moved)"
          % (name, D, H, Hp, g, M, lay["lp"].shape[1], err, moved))
    assert err <= RTOL
    if name.startswith("gsc"):
        assert np.array_equal(S != 0, S_want != 0)
        assert R.row_rel_err(S.reshape(M * N, H), S_want.reshape(M * N, H)) <= RTOL
    else:
        assert np.array_equal(S, S_want)
    assert np.array_equal(m.sample_posterior(p, {"y": Y}, n_samples=M, uniforms=U, **kw), Ys)      # without latents: same bits


BITS = [("bsc_mu", 24, 12, 5, 3), ("mca", 24, 12, 5, 3), ("mmca", 24, 12, 5, 3), ("dsc4", 24, 12, 5, 3), ("tsc", 24, 12, 5, 3),
        ("gsc_scalar", 24, 12, 5, 3), ("mog_diagonal", 24, 9, 0, 0), ("mog_full", 24, 9, 0, 0), ("mop_A", 24, 9, 0, 0)]


@pytest.mark.parametrize("name,D,H,Hp,g", BITS)
def test_bit_guarantees(dev, name, D, H, Hp, g):
    """A second call, the deterministic library, a row permutation with U / E permuted along, a shard, a forced small chunk,
    device input and device output: equal bits."""
    import torch
    from prosper_amd.em.camodels._device import DeviceArray
    rng = np.random.RandomState(13)
    N, M = 300, 5
    m, p, Y = _make(name, rng, D, H, N, Hp, g)
    U = rng.uniform(size=(N, M))
    kw = _normals(m, name, rng, N, M)
    E = kw.get("normals")
    sub = lambda sel: ({"normals": E[sel]} if E is not None else {})
    a, s = m.sample_posterior(p, {"y": Y}, n_samples=M, uniforms=U, latents=True, **kw)
    assert np.isfinite(a).all()
    b, t = m.sample_posterior(p, {"y": Y}, n_samples=M, uniforms=U, latents=True, **kw)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(s, t)
    if hasattr(m, "deterministic"):
        m.deterministic = True
        np.testing.assert_array_equal(m.sample_posterior(p, {"y": Y}, n_samples=M, uniforms=U, **kw), a)
        m.deterministic = False
    perm = rng.permutation(N)
    np.testing.assert_array_equal(m.sample_posterior(p, {"y": Y[perm]}, n_samples=M, uniforms=U[perm], **sub(perm)), a[:, perm])
    sh = slice(77, 201)
    np.testing.assert_array_equal(m.sample_posterior(p, {"y": Y[sh]}, n_samples=M, uniforms=U[sh], **sub(sh)), a[:, sh])
    m.sample_chunk_rows = 7
    c, u = m.sample_posterior(p, {"y": Y}, n_samples=M, uniforms=U, latents=True, **kw)
    m.sample_chunk_rows = None
    np.testing.assert_array_equal(c, a)
    np.testing.assert_array_equal(u, s)
    kd = {"normals": DeviceArray(torch.from_numpy(E).to(dev))} if E is not None else {}
    d = m.sample_posterior(p, {"y": torch.from_numpy(Y).to(dev)}, n_samples=M, uniforms=torch.from_numpy(U).to(dev), device=True,
                           **kd)
    assert isinstance(d, DeviceArray) and d.tensor.is_cuda and d.shape == (M, N, D)
    np.testing.assert_array_equal(np.asarray(d), a)


@pytest.mark.parametrize("name", ["bsc_mu", "mca", "mmca"])
def test_masked_draws_ignore_what_unobserved_entries_hold(dev, name):
    rng = np.random.RandomState(21)
    D, H, N, M = 20, 10, 120, 4
    m, p, Y = _make(name, rng, D, H, N, 5, 3)
    mask = rng.uniform(size=(N, D)) < 0.6
    mask[3] = False                                   # a row with nothing observed: a draw from the prior's truncated states
    U = rng.uniform(size=(N, M))
    ref = None
    for fill in (0.0, np.nan, np.inf, 1e300):
        Yf = np.where(mask, Y, fill)
        got = m.sample_posterior(p, {"y": Yf, "mask": mask}, n_samples=M, uniforms=U)
        assert got.shape == (M, N, D) and np.isfinite(got).all()
        if ref is None:
            ref = got
        np.testing.assert_array_equal(got, ref)
    # all observed: the bits of the unmasked E-step's draws need not match (another kernel), the distribution does: same states
    # for uniforms away from the edges -- checked through the statistical tie below


STAT = [("bsc_mu", 20, 10, 5, 3), ("mca", 20, 10, 5, 3), ("mmca", 20, 10, 5, 3), ("dsc4", 20, 10, 5, 3), ("tsc", 20, 10, 5, 3),
        ("gsc_scalar", 20, 10, 4, 3), ("mog_diagonal", 20, 6, 0, 0), ("mop", 20, 6, 0, 0), ("bsc_masked", 20, 10, 5, 3),
        ("mca_masked", 20, 10, 5, 3)]


@pytest.mark.parametrize("name,D,H,Hp,g", STAT)
def test_statistical_tie_to_reconstruct_and_its_variance(dev, name, D, H, Hp, g):
    """N = 8 rows, M = 4096 seeded draws: |mean_m Ys - yhat| <= 6 sqrt(V / M) + 1e-12 max |yhat| per pixel, yhat and V from
    reconstruct(variance=True) (module docstring: the bound is derived)."""
    masked = name.endswith("_masked")
    base = {"bsc_masked": "bsc_mu", "mca_masked": "mca"}.get(name, name)
    rng = np.random.RandomState(17)
    N, M = 8, 4096
    m, p, Y = _make(base, rng, D, H, N, Hp, g)
    data = {"y": Y}
    if masked:
        data["mask"] = rng.uniform(size=(N, D)) < 0.6
    yhat, V = m.reconstruct(p, dict(data), variance=True)
    Ys = m.sample_posterior(p, dict(data), n_samples=M, seed=5)
    mean = Ys.mean(axis=0)
    bound = 6.0 * np.sqrt(V / M) + 1e-12 * np.abs(yhat).max()
    worst = float((np.abs(mean - yhat) / bound).max())
    print("sample_posterior %-12s |mean - yhat| / bound: largest %.3f over %d pixels" % (name, worst, N * D))
    assert worst <= 1.0


# (the mixture in two dimensions: its components overlap, so that other uniforms do give other draws)
@pytest.mark.parametrize("name,D,H,Hp,g", [("bsc", 16, 10, 5, 3), ("gsc_scalar", 16, 10, 4, 3), ("mog_diagonal", 2, 6, 0, 0)])
def test_seeded_path(dev, name, D, H, Hp, g):
    import torch
    rng = np.random.RandomState(2)
    N, M = 50, 6
    m, p, Y = _make(name, rng, D, H, N, Hp, g)
    a = m.sample_posterior(p, {"y": Y}, n_samples=M, seed=3)
    np.testing.assert_array_equal(m.sample_posterior(p, {"y": Y}, n_samples=M, seed=3), a)
    assert not np.array_equal(m.sample_posterior(p, {"y": Y}, n_samples=M, seed=4), a)
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    U = torch.rand((N, M), generator=gen, device=dev, dtype=torch.float64)
    kw = {}
    if name.startswith("gsc"):
        kw["normals"] = torch.randn((N, M, g), generator=gen, device=dev, dtype=torch.float64)
    np.testing.assert_array_equal(m.sample_posterior(p, {"y": Y}, n_samples=M, uniforms=U, **kw), a)
    np.testing.assert_array_equal(m.sample_posterior(p, {"y": Y}, n_samples=M, uniforms=U.cpu().numpy(), **kw), a)
    b = m.sample_posterior(p, {"y": Y}, n_samples=M)                 # no seed: fresh entropy
    assert b.shape == a.shape and np.isfinite(b).all()


@pytest.mark.parametrize("name", ["bsc", "mca", "dsc3", "tsc", "gsc_full", "mog_diagonal", "mop"])
def test_nan_row_and_device_uniforms_out_of_range(dev, name):
    import torch
    rng = np.random.RandomState(11)
    N, M, D = 70, 3, 6
    m, p, Y = _make(name, rng, D, 5, N, 3, 2)
    U = rng.uniform(size=(N, M))
    kw = _normals(m, name, rng, N, M)
    clean, s_clean = m.sample_posterior(p, {"y": Y}, n_samples=M, uniforms=U, latents=True, **kw)
    Yn = Y.copy()
    Yn[13, 2] = np.nan
    rows, s = m.sample_posterior(p, {"y": Yn}, n_samples=M, uniforms=U, latents=True, **kw)
    assert np.isnan(rows[:, 13]).all() and np.isnan(s[:, 13]).all()
    np.testing.assert_array_equal(np.delete(rows, 13, axis=1), np.delete(clean, 13, axis=1))
    np.testing.assert_array_equal(np.delete(s, 13, axis=1), np.delete(s_clean, 13, axis=1))
    # a DEVICE array of uniforms is not inspected: values outside [0, 1) and NaN are clamped into it by the kernel
    Ud = torch.from_numpy(U).to(dev)
    Ud[5, 0], Ud[6, 1], Ud[7, 2] = 1.5, -0.5, float("nan")
    out = m.sample_posterior(p, {"y": Y}, n_samples=M, uniforms=Ud, **kw)
    assert np.isfinite(out).all()
    Uc = U.copy()
    Uc[5, 0], Uc[6, 1], Uc[7, 2] = SR.U_MAX, 0.0, 0.0
    np.testing.assert_array_equal(out, m.sample_posterior(p, {"y": Y}, n_samples=M, uniforms=Uc, **kw))


def test_refusals_return_nothing_and_launch_nothing(dev):
    from prosper_amd import _lib
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    rng = np.random.RandomState(6)
    for name in ("dsc3", "tsc", "gsc_scalar", "mog_diagonal", "mop"):
        m, p, Y = _make(name, rng, 8, 6, 10, 3, 2)
        calls = TR._entries(m) if hasattr(m, "_call") else []
        with pytest.raises(NotImplementedError, match="mask"):
            m.sample_posterior(p, {"y": Y, "mask": np.ones_like(Y, dtype=bool)})
        assert not calls
    m, p, Y = _make("bsc", rng, 8, 6, 10, 3, 2)
    calls = TR._entries(m)
    for bad in (dict(n_samples=0), dict(n_samples=2, uniforms=np.zeros((10, 3))), dict(uniforms=np.full((10, 1), 1.0))):
        with pytest.raises(ValueError):
            m.sample_posterior(p, {"y": Y}, **bad)
    assert not calls
    D, N = 16, 12
    for H, Hp, ok in ((40, 16, True), (40, 17, False)):
        p = {"W": rng.normal(size=(D, H)), "pi": 2.0 / H, "sigma": 1.0}
        Y = rng.normal(size=(N, D))
        if ok:
            assert BSC_ET(D, H, Hp, 2).sample_posterior(p, {"y": Y}).shape == (1, N, D)
        else:
            with pytest.raises(_lib.HipError):
                BSC_ET(D, H, Hp, 2).sample_posterior(p, {"y": Y})
    for D, ok in ((1024, True), (1025, False)):
        p = {"W": rng.uniform(0.5, 2.0, size=(D, 8)), "pi": 0.2, "sigma": 1.0}
        Y = rng.uniform(0, 2, size=(5, D))
        if ok:
            assert MCA_ET(D, 8, 4, 2).sample_posterior(p, {"y": Y}).shape == (1, 5, D)
        else:
            with pytest.raises(_lib.HipError):
                MCA_ET(D, 8, 4, 2).sample_posterior(p, {"y": Y})


@pytest.mark.parametrize("name", ["bsc", "mca", "gsc_scalar"])
def test_second_trip_of_the_row_loops(dev, name):
    """N = 8269 (tests/test_sample_abi_gpu.py: 8192 rows per trip of the state kernel; M = 4: 33076 > 32768 pairs per trip of
    the decode kernels).  The rows from 100 before the boundary to the end against NumPy on an E-step of those rows alone;
    everything bit for bit against 4096-row shards given the matching rows of U / E."""
    rng = np.random.RandomState(900 + len(name))
    D, H, Hp, g, N, M = 8, 6, 4, 2, 8269, 4
    m, p, Y = _make(name, rng, D, H, N, Hp, g)
    U = rng.uniform(size=(N, M))
    kw = _normals(m, name, rng, N, M)
    E = kw.get("normals")
    tail = slice(8192 - 100, N)
    lay = _layout(m, name, p, Y[tail])
    U[tail], _ = SR.nudge(U[tail], SR.cdfs(lay["lp"], **lay["kw"]))
    got = m.sample_posterior(p, {"y": Y}, n_samples=M, uniforms=U, **kw)
    assert got.shape == (M, N, D) and np.isfinite(got).all()
    want, _ = lay["draw"](SR.draw_states(lay["lp"], U[tail], **lay["kw"]), E[tail] if E is not None else None)
    assert _rel(got[:, tail], want) <= RTOL
    shards = np.concatenate([m.sample_posterior(p, {"y": Y[i:i + 4096]}, n_samples=M, uniforms=U[i:i + 4096],
                                                **({"normals": E[i:i + 4096]} if E is not None else {}))
                             for i in range(0, N, 4096)], axis=1)
    assert np.array_equal(shards.view(np.uint64), got.view(np.uint64))


def test_training_state_is_untouched(dev):
    """A call between two EM steps leaves the trajectory as it was (deterministic library: equal bits)."""
    rng = np.random.RandomState(14)
    D, H, N = 20, 10, 1200
    _, p, Y, _, _ = TR._problem("bsc", rng, D, H, N + 200, 5, 3)
    p = dict(p, W=p["W"] * rng.uniform(0.9, 1.1, size=p["W"].shape))

    def train(interleave):
        m = TR._problem("bsc", np.random.RandomState(0), D, H, 4, 5, 3)[0]
        m.deterministic = True
        a = TR._schedule(4)
        q = {k: np.array(v, copy=True) for k, v in p.items()}
        for _ in range(4):
            q = m.step(a, q, {"y": Y[:N]})
            if interleave:
                out = m.sample_posterior({k: np.array(v, copy=True) for k, v in q.items()}, {"y": Y[N:]}, n_samples=2, seed=1)
                assert np.isfinite(out).all() and (m.Hprime, m.gamma) == (5, 3)
            a.next()
        return q
    ref, got = train(False), train(True)
    for k in ref:
        np.testing.assert_array_equal(ref[k], got[k], err_msg=k)


def test_two_ranks_over_gloo(dev):
    """tests/sample_world2_gpu_worker.py: two processes, a world_size-2 gloo group on the one GPU; each rank's draws equal the
    corresponding rows of a one-rank call given the matching U (and E), bit for bit."""
    import os
    import socket
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    worker = os.path.join(here, "sample_world2_gpu_worker.py")
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
