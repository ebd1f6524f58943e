"""k-means++ seeding without a GPU: the properties of the NumPy restatement tests/seeding_reference.py that the
GPU tests compare the kernels with, the refusals that need no device, and pm_seed_plan / pm_seed_work_len against the
documented rule."""
import ctypes

import numpy as np
import pytest

import seeding_reference as SR


def _data(seed, N, D, distinct=None):
    rng = np.random.RandomState(seed)
    Y = rng.normal(size=(N, D)) * 3.0
    if distinct is not None:
        Y = Y[rng.randint(0, distinct, size=N)]
    return Y


@pytest.mark.parametrize("N,D,H", [(1, 1, 1), (40, 3, 40), (97, 5, 12), (300, 16, 8), (130, 70, 9)])
def test_distinct_indices_zero_distance_and_monotone_potential(N, D, H):
    Y = _data(N + D, N, D)
    rng = np.random.RandomState(H)
    u = rng.uniform(size=H)
    centres, idx, pot, (dist, B, Q) = SR.kmeanspp([Y], H, u)
    assert len(set(idx.tolist())) == H and (idx >= 0).all() and (idx < N).all()
    np.testing.assert_array_equal(centres, Y[idx])
    assert (dist[idx] == 0.0).all() and (dist >= 0.0).all()
    assert (np.diff(pot) <= 0.0).all() and np.isfinite(pot).all()
    assert idx[0] == min(int(np.floor(u[0] * N)), N - 1)
    # the final distances are the minimum over the chosen centres, each in the kernel's order
    g = SR.plan(N, D)[2]
    want = np.min([SR.distances(Y, Y[i], g) for i in idx], axis=0)
    np.testing.assert_array_equal(dist, want)


def test_distance_order_is_the_documented_one():
    """g partial sums over d = l, l + g, ..., then butterflies o = g/2 ... 1: written out for one row per g."""
    rng = np.random.RandomState(3)
    for D in (1, 2, 3, 5, 33, 64, 65, 200):
        y, c = rng.normal(size=D), rng.normal(size=D)
        g = SR.plan(7, D)[2]
        assert g == min(64, 1 << int(np.ceil(np.log2(D)))) if D > 1 else g == 1
        v = [0.0] * g
        for l in range(g):
            for d in range(l, D, g):
                t = y[d] - c[d]
                v[l] = v[l] + t * t
        o = g // 2
        while o:
            v = [v[l] + v[l ^ o] for l in range(g)]
            o //= 2
        assert SR.distances(y[None, :], c, g)[0] == v[0]
        assert all(x == v[0] for x in v)


def test_zero_rows_are_never_drawn_at_the_ends_of_the_interval():
    rng = np.random.RandomState(5)
    for N in (17, 64, 1025):
        dist = rng.uniform(0.5, 2.0, size=N)
        dist[rng.uniform(size=N) < 0.7] = 0.0
        dist[0] = dist[-1] = 0.0
        rpb = SR.plan(N, 4)[0]
        B, Q = SR.block_sums(dist, rpb)
        for u in (0.0, np.nextafter(1.0, 0.0), 0.5, np.nextafter(0.0, 1.0)):
            n = SR.pick(dist, B, Q, rpb, u)
            assert n >= 0 and dist[n] > 0.0, (N, u)
        assert SR.pick(dist, B, Q, rpb, 0.0) == int(np.nonzero(dist > 0)[0][0])
        assert SR.pick(dist, B, Q, rpb, np.nextafter(1.0, 0.0)) == int(np.nonzero(dist > 0)[0][-1])


def test_integer_distances_give_searchsorted_on_the_exact_cumsum():
    rng = np.random.RandomState(8)
    for N in (5, 16, 17, 333, 4099):
        dist = rng.randint(0, 9, size=N).astype(np.float64)
        rpb = SR.plan(N, 4)[0]
        B, Q = SR.block_sums(dist, rpb)
        cum = np.cumsum(dist)
        assert Q[-1] == cum[-1]
        for u in np.concatenate([rng.uniform(size=40), [0.0, 0.25, 0.5, 0.75]]):
            t = u * cum[-1]
            assert SR.pick(dist, B, Q, rpb, u) == int(np.searchsorted(cum, t, side="right"))
        # t exactly on a block boundary: the first row past it with a positive distance
        for b in range(len(Q) - 1):
            u = Q[b] / Q[-1]
            if u * Q[-1] == Q[b]:
                assert SR.pick(dist, B, Q, rpb, u) == int(np.searchsorted(cum, Q[b], side="right"))


def test_integer_data_seeding_is_exact():
    rng = np.random.RandomState(9)
    Y = rng.randint(-6, 7, size=(200, 7)).astype(np.float64)
    u = rng.uniform(size=6)
    _, idx, pot, (dist, B, Q) = SR.kmeanspp([Y], 6, u)
    want = np.min([((Y - Y[i]) ** 2).sum(1) for i in idx], axis=0)
    np.testing.assert_array_equal(dist, want)
    assert pot[-1] == want.sum()


def test_exhausted_data_returns_minus_one_from_the_right_round():
    Y = _data(2, 50, 4, distinct=3)
    u = np.random.RandomState(0).uniform(size=6)
    _, idx, pot, _ = SR.kmeanspp([Y], 6, u)
    assert (idx[:3] >= 0).all() and (idx[3:] == -1).all()
    assert len({tuple(Y[i]) for i in idx[:3]}) == 3
    assert (pot[:2] > 0).all() and (pot[2:] == 0.0).all()


def test_two_shards_follow_the_rank_order_rule():
    """Global indices; a shard of one rank reproduces the one-rank run when the other holds no potential."""
    rng = np.random.RandomState(4)
    Y = _data(11, 90, 6)
    u = rng.uniform(size=7)
    c2, i2, p2, _ = SR.kmeanspp([Y[:50], Y[50:]], 7, u)
    assert len(set(i2.tolist())) == 7 and (np.diff(p2) <= 0).all()
    np.testing.assert_array_equal(c2, Y[i2])
    assert i2[0] == min(int(np.floor(u[0] * 90)), 89)


def test_refusals_that_need_no_device():
    from prosper_amd.utils.seeding import kmeanspp
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.em.mixturemodels.MoP import MoP
    Y = _data(1, 20, 4)
    for bad in (dict(H=0), dict(H=21), dict(H=-3),
                dict(H=3, uniforms=np.zeros(4)), dict(H=3, uniforms=np.zeros((3, 1))),
                dict(H=3, uniforms=np.array([0.1, 1.0, 0.2])), dict(H=3, uniforms=np.array([0.1, -1e-9, 0.2])),
                dict(H=3, uniforms=np.array([0.1, np.nan, 0.2])),
                dict(H=3, uniforms=np.array([0.1, 0.5, 0.2]), seed=1)):
        with pytest.raises(ValueError):
            kmeanspp(Y, **bad)
    with pytest.raises(ValueError):
        kmeanspp(Y[0], 1, uniforms=np.zeros(1))
    for m in (MoG(5, 3, sigmas_sq_type='diagonal'), MoG(5, 3), MoP(5, 3)):
        with pytest.raises(ValueError, match="must be"):
            m.kmeanspp_init({'y': Y}, uniforms=np.zeros(3))
        with pytest.raises(ValueError):
            m.kmeanspp_init({'y': Y[:, :1].repeat(5, 1)}, seed=1, uniforms=np.zeros(3))


def test_component_analysis_models_have_no_seeding():
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    assert not hasattr(BSC_ET, "kmeanspp_init")


@pytest.mark.parametrize("N", [1, 2, 1023, 1024, 1025, 10 ** 6])
@pytest.mark.parametrize("D", [1, 2, 63, 64, 65, 4096])
def test_plan_and_work_len_follow_the_documented_rule(N, D):
    from prosper_amd import _lib
    lib = _lib.load()
    assert lib.pm_version() >= 1036 and _lib.MIN_VERSION >= 1036 and _lib.load(True).pm_version() >= 1036
    out = (ctypes.c_int32 * 8)()
    assert lib.pm_seed_plan(N, D, out) == 0
    rpb, nb, g, rpw = SR.plan(N, D)
    assert list(out)[:6] == [rpb, nb, g, rpw, nb, 4]
    assert out[6] == 8 * (D + D % 2) and out[7] == -(-((D + 1) // 2) // max(g // 2, 1))
    assert nb <= 1024 and (nb - 1) * rpb < N <= nb * rpb
    assert lib.pm_seed_work_len(N) == 2 * nb == SR.work_len(N)
    assert {1: (1, 1), 2: (2, 1), 1023: (16, 64), 1024: (16, 64), 1025: (16, 65), 10 ** 6: (977, 1024)}[N] == (rpb, nb)
    assert {1: (1, 64), 2: (2, 64), 63: (64, 2), 64: (64, 2), 65: (64, 2), 4096: (64, 2)}[D] == (g, rpw)


def test_plan_refusals():
    from prosper_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int32 * 8)()
    assert lib.pm_seed_plan(0, 4, out) == -1 and lib.pm_seed_plan(4, 0, out) == -1 and lib.pm_seed_plan(4, 4, None) == -1
    assert lib.pm_seed_plan(4, 6145, out) == -2 and lib.pm_seed_plan((1 << 40) + 1, 4, out) == -2
    assert lib.pm_seed_plan(4, 6144, out) == 0
    assert lib.pm_seed_work_len(0) == 2 and lib.pm_seed_work_len(-1) == -1
    # every launcher returns before it touches a device
    assert lib.pm_seed_update_f64(None, 4, 4, 4, None, 4, 1, None, 1, None, None, None, None) == -1
    assert lib.pm_seed_update_f64(8, 3, 4, 4, 8, 4, 1, None, 1, 8, 8, None, None) == -1          # ldy < D
    assert lib.pm_seed_update_f64(8, 4, 4, 4, 8, 3, 1, None, 1, 8, 8, None, None) == -1          # ldc < D
    assert lib.pm_seed_update_f64(8, 4, 4, 4, 8, 4, 0, None, 1, 8, 8, None, None) == -1          # no centre rows
    assert lib.pm_seed_update_f64(8, 7000, 4, 7000, 8, 7000, 1, None, 1, 8, 8, None, None) == -2
    assert lib.pm_seed_update_f64(8, 4, 0, 4, 8, 4, 1, None, 1, 8, 8, None, None) == 0           # N == 0: nothing
    assert lib.pm_seed_pick_f64(None, 4, 8, None, 0.0, 0.5, 8, None) == -1
    assert lib.pm_seed_pick_f64(8, -1, 8, None, 0.0, 0.5, 8, None) == -1
    assert lib.pm_seed_pick_f64(8, 0, 8, None, 0.0, 0.5, 8, None) == 0
    assert lib.pm_seed_gather_f64(8, 4, 4, 4, None, 2, 8, 4, None) == -1
    assert lib.pm_seed_gather_f64(8, 4, 4, 4, 8, 2, 8, 3, None) == -1
    assert lib.pm_seed_gather_f64(8, 4, 4, 4, 8, 0, 8, 4, None) == 0
