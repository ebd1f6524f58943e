"""k-means++ seeding through the public interface: ``utils.seeding.kmeanspp`` and ``kmeanspp_init`` of MoG
(diagonal, full) and MoP against tests/seeding_reference.py.  Every comparison is exact: the kernels' summation orders are
pinned, so indices and potentials are compared bit for bit."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import seeding_reference as SR

pytestmark = pytest.mark.gpu


class An(dict):
    def __missing__(self, k):
        return 0.0

    def as_dict(self):
        return dict(self)


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _case(N, D, H, seed=0):
    rng = np.random.RandomState(100 * seed + N + D + H)
    return rng.normal(size=(N, D)) * 2.0 + rng.normal(size=(8, D))[rng.randint(0, 8, size=N)] * 4.0, rng.uniform(size=H)


REF = {}


def _ref(N, D, H):
    """The reference of a case, computed once and shared."""
    if (N, D, H) not in REF:
        Y, u = _case(N, D, H)
        REF[(N, D, H)] = (Y, u) + SR.kmeanspp([Y], H, u)[:3]
    return REF[(N, D, H)]


def _equal(got, want, what=""):
    c, i, p = got
    assert np.array_equal(i, want[1]) and i.dtype == np.int64, (what, i, want[1])
    assert np.array_equal(_bits(p), _bits(want[2])), (what, "potential")
    assert np.array_equal(_bits(np.asarray(c)), _bits(want[0])) and np.asarray(c).shape == want[0].shape, (what, "centres")


@pytest.mark.parametrize("N,D,H", [(300, 16, 8), (1025, 65, 20), (4099, 200, 5)])
def test_kmeanspp_matches_the_reference(dev, N, D, H):
    from prosper_amd.utils.seeding import kmeanspp
    Y, u, c, i, p = _ref(N, D, H)
    assert len(set(i.tolist())) == H and (np.diff(p) <= 0).all()
    _equal(kmeanspp(Y, H, uniforms=u), (c, i, p))


def test_float32_input_is_converted_once(dev):
    import torch
    from prosper_amd.utils.seeding import kmeanspp
    Y, u = _case(300, 16, 8, seed=1)
    Y32 = Y.astype(np.float32)
    want = SR.kmeanspp([Y32.astype(np.float64)], 8, u)[:3]
    _equal(kmeanspp(Y32, 8, uniforms=u), want, "numpy f32")
    _equal(kmeanspp(torch.from_numpy(Y32).to(dev), 8, uniforms=u), want, "device f32")


def test_same_bits_from_every_form_of_the_input_and_both_libraries(dev):
    import torch
    from prosper_amd.em.camodels._device import DeviceArray
    from prosper_amd.utils.seeding import kmeanspp
    Y, u, c, i, p = _ref(1025, 65, 20)
    want = (c, i, p)
    Yd = torch.from_numpy(Y).to(dev)
    wide = torch.full((1025, 70), float("nan"), dtype=torch.float64, device=dev)
    wide[:, :65] = Yd
    for what, arg in (("numpy", Y), ("again", Y), ("torch cpu", torch.from_numpy(Y)), ("torch device", Yd),
                      ("DeviceArray", DeviceArray(Yd)), ("a view with a row stride of 70", wide[:, :65]),
                      ("fortran order", np.asfortranarray(Y))):
        _equal(kmeanspp(arg, 20, uniforms=u), want, what)
    _equal(kmeanspp(Y, 20, uniforms=u, deterministic=True), want, "libprosper_hip_det.so")
    _equal(kmeanspp(Y, 20, uniforms=torch.from_numpy(u).to(dev)), want, "device uniforms")
    cd, i2, p2 = kmeanspp(Yd, 20, uniforms=u, device=True)
    assert isinstance(cd, DeviceArray) and cd.tensor.is_cuda
    _equal((cd.tensor.cpu().numpy(), i2, p2), want, "device=True")


def test_seeded_path(dev):
    import torch
    from prosper_amd.utils.seeding import kmeanspp
    Y, _ = _case(300, 16, 8)
    a = kmeanspp(Y, 8, seed=3)
    _equal(kmeanspp(Y, 8, seed=3), a, "same seed")
    assert not np.array_equal(kmeanspp(Y, 8, seed=4)[1], a[1])
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    u = torch.rand(8, generator=g, device=dev, dtype=torch.float64)
    _equal(kmeanspp(Y, 8, uniforms=u), a, "the generator's uniforms")
    _equal(a, SR.kmeanspp([Y], 8, u.cpu().numpy())[:3], "reference")
    b = kmeanspp(Y, 8)                                    # no seed: fresh entropy
    assert len(set(b[1].tolist())) == 8


def _models(D, H):
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.em.mixturemodels.MoP import MoP
    return [("mog_diagonal", lambda: MoG(D, H, sigmas_sq_type='diagonal')), ("mog_full", lambda: MoG(D, H, sigmas_sq_type='full')),
            ("mop", lambda: MoP(D, H))]


@pytest.mark.parametrize("k", [0, 1, 2])
def test_kmeanspp_init(dev, k):
    N, D, H = 300, 16, 8
    name, make = _models(D, H)[k]
    Y, u = _case(N, D, H)
    if name == "mop":
        Y = np.floor(np.abs(Y)) + (np.abs(Y) > 1.0) * np.abs(Y) % 1.0     # counts with zeros (a zero rate has no logarithm)
        assert (Y == 0.0).any() and len(np.unique(Y, axis=0)) == N
    want = SR.kmeanspp([Y], H, u)[:3]
    m = make()
    state = np.random.get_state()
    p = m.kmeanspp_init({'y': Y}, uniforms=u)
    after = np.random.get_state()
    assert all(np.array_equal(a, b) for a, b in zip(state, after)), "kmeanspp_init drew from NumPy's generator"
    assert np.array_equal(m.seed_indices, want[1]) and np.array_equal(_bits(m.seed_potential), _bits(want[2]))
    chosen = Y[want[1]]
    if name == "mop":                                     # MoP: rates are positive, a zero count becomes the M-step's floor
        chosen = np.maximum(chosen, np.finfo(np.float64).eps)
        assert (p['W'] > 0).all() and (Y[want[1]] == 0.0).any()
    checked = m.check_params({'W': chosen.T.copy(), **{k2: v for k2, v in p.items() if k2 != 'W'}})
    assert p['W'].shape == (D, H) and np.array_equal(_bits(p['W']), _bits(checked['W']))
    for h in range(H):
        assert np.array_equal(_bits(p['W'][:, h]), _bits(chosen[h]))
    std = make().standard_init({'y': Y})
    np.random.set_state(state)
    assert sorted(std) == sorted(p)
    for key in std:
        if key != 'W':
            assert np.array_equal(_bits(std[key]), _bits(p[key])) and std[key].shape == p[key].shape, key
    # a fresh model, and the seeded form
    p2 = make().kmeanspp_init({'y': Y}, uniforms=u)
    assert all(np.array_equal(_bits(p[key]), _bits(p2[key])) for key in p)
    p3, p4 = make().kmeanspp_init({'y': Y}, seed=5), make().kmeanspp_init({'y': Y}, seed=5)
    assert np.array_equal(_bits(p3['W']), _bits(p4['W']))
    new = m.step(An(T=1.0), {key: np.array(v, copy=True) for key, v in p.items()}, {'y': Y})
    assert all(np.isfinite(np.asarray(v)).all() for v in new.values()), name


def test_a_call_between_two_em_steps_leaves_the_trajectory_alone(dev):
    """The seeding keeps its buffers to itself: the training shard and workspaces of the model are as they were.  (The mixture
    kernels hold no atomics; the seeding runs on the deterministic library here, as the other order-of-calls tests do.)"""
    from prosper_amd.em.mixturemodels.MoG import MoG
    N, D, H = 400, 12, 6
    Y, u = _case(N, D, H)

    def train(interleave):
        m = MoG(D, H, sigmas_sq_type='diagonal')
        m.deterministic = True
        np.random.seed(3)
        p = m.standard_init({'y': Y})
        for _ in range(3):
            p = m.step(An(T=1.0), p, {'y': Y})
            if interleave:
                q = m.kmeanspp_init({'y': Y[:200]}, uniforms=u)
                assert np.isfinite(q['W']).all()
        return p
    ref, got = train(False), train(True)
    for key in ref:
        assert np.array_equal(_bits(ref[key]), _bits(got[key])), key


def test_refusals_launch_nothing(dev, monkeypatch):
    from prosper_amd import _lib
    from prosper_amd.utils.seeding import kmeanspp
    from prosper_amd.em.mixturemodels.MoG import MoG
    calls = []
    orig = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **kw: (calls.append(name), orig(name, *a, **kw))[1])
    Y, _ = _case(40, 6, 4)
    for bad in (dict(H=0), dict(H=41), dict(H=4, uniforms=np.zeros(5)), dict(H=4, uniforms=np.zeros((4, 1))),
                dict(H=4, uniforms=np.array([0.1, 1.0, 0.2, 0.3])), dict(H=4, uniforms=np.array([0.1, -0.5, 0.2, 0.3])),
                dict(H=4, uniforms=np.array([0.1, np.nan, 0.2, 0.3])), dict(H=4, uniforms=np.full(4, 0.5), seed=2)):
        with pytest.raises(ValueError):
            kmeanspp(Y, **bad)
    m = MoG(7, 4, sigmas_sq_type='diagonal')
    with pytest.raises(ValueError, match="must be"):
        m.kmeanspp_init({'y': Y}, seed=1)
    with pytest.raises(ValueError):
        MoG(6, 4).kmeanspp_init({'y': Y}, seed=1, uniforms=np.full(4, 0.5))
    assert not calls
    kmeanspp(Y, 4, seed=1)                                # (the spy does see a call that runs)
    assert "pm_seed_update_f64" in calls and "pm_seed_pick_f64" in calls


def test_duplicate_rows_and_non_finite_data_raise_after_the_rounds(dev):
    from prosper_amd.utils.seeding import kmeanspp
    rng = np.random.RandomState(7)
    rows = rng.normal(size=(3, 5))
    Y = rows[rng.randint(0, 3, size=60)]
    Y[:3] = rows
    u = rng.uniform(size=5)
    assert len(set(kmeanspp(Y, 3, uniforms=u[:3])[1].tolist())) == 3
    with pytest.raises(ValueError, match="round 3"):
        kmeanspp(Y, 5, uniforms=u)
    for bad in (np.nan, np.inf):
        Z = rng.normal(size=(60, 5))
        Z[17, 2] = bad
        with pytest.raises(ValueError, match="not finite"):
            kmeanspp(Z, 4, uniforms=u[:4])


def _spawn(worker, world, extra=None):
    here = os.path.dirname(os.path.abspath(__file__))
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    procs = []
    for rank in range(world):
        e = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                 RANK=str(rank), WORLD_SIZE=str(world), **(extra or {}))
        procs.append(subprocess.Popen([sys.executable, os.path.join(here, worker)], env=e, stdout=subprocess.PIPE,
                                      stderr=subprocess.PIPE, text=True))
    outs = []
    try:
        for pr in procs:
            outs.append(pr.communicate(timeout=300))
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
    for rank, (pr, (out, err)) in enumerate(zip(procs, outs)):
        assert pr.returncode == 0 and ("ok %d" % rank) in out, "rank %d:\n%s\n%s" % (rank, out, err[-3000:])


def test_two_ranks_over_gloo(dev):
    """tests/seeding_world2_gpu_worker.py: two processes, a world_size-2 gloo group on the one GPU; both ranks hold identical
    centres, equal to the reference on the two shards with the rank-order rule; the indices are global."""
    _spawn("seeding_world2_gpu_worker.py", 2)


def test_forced_collectives_on_one_rank_give_the_one_rank_bits(dev):
    """PM_FORCE_COLLECTIVES=1 in a one-rank gloo group runs the collective form: the bits of the enqueued one-rank loop."""
    _spawn("seeding_world2_gpu_worker.py", 1, {"PM_FORCE_COLLECTIVES": "1"})
