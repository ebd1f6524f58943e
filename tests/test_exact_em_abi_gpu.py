"""pm_moments_exact_lin_f64 (include/prosper_hip.h) through the C ABI against the NumPy enumeration of
tests/exact_em_reference.py, to the enumeration kernels' 1e-11 of the row's largest entry.  Every case names the cell of
pm_moments_exact_plan it confirms: [L, CH, chunks, R, pinned sweeps, lo-lo pairs, ranges of the pair sweeps]."""
import ctypes

import numpy as np
import pytest

import exact_em_reference as X
from test_exact_em_cpu import closed_form

pytestmark = pytest.mark.gpu

RTOL = 1e-11
SENTINEL = -12345.678


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _up(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def _plan(N, D, K, H):
    from prosper_amd import _lib
    out = (ctypes.c_int64 * 12)()
    assert _lib.load().pm_moments_exact_plan(N, D, K, H, out) == 0
    return list(out)


def _run(dev, Y, W, sigma, values, logp, mu=None, det=False, pad=(0, 0, 0), recon=False):
    """(E, C, v) of the entry; ``pad`` = extra doubles per row of Y, E and C (the buffers are filled with a sentinel, which must
    survive past the row width).  ``recon``: E of pm_recon_exact_lin_f64 on the same arguments instead."""
    import torch
    from prosper_amd import _lib
    lib = _lib.load(det)
    Y = np.asarray(Y, dtype=np.float64)
    N, D = Y.shape
    H, K = W.shape[1], len(values)
    npair = H * (H + 1) // 2
    ldy, lde, ldc = D + pad[0], H + pad[1], npair + pad[2]
    Yd = torch.full((N, ldy), float("nan"), dtype=torch.float64, device=dev)
    Yd[:, :D] = _up(Y, dev)
    P, G = _up(W / sigma ** 2, dev), _up(W.T @ W / sigma ** 2, dev)
    lp, vals = _up(logp, dev), _up(values, dev)
    mud = _up(mu, dev) if mu is not None else None
    E = torch.full((N, lde), SENTINEL, dtype=torch.float64, device=dev)
    if recon:
        work = torch.empty(int(lib.pm_recon_exact_work_len(N, H, D)), dtype=torch.float64, device=dev)
        rc = lib.pm_recon_exact_lin_f64(_ptr(Yd), ldy, _ptr(mud), _ptr(P), _ptr(G), _ptr(lp), _ptr(vals), K, N, D, H, _ptr(E),
                                        lde, _ptr(work), None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        return E.cpu().numpy()[:, :H]
    C = torch.full((N, ldc), SENTINEL, dtype=torch.float64, device=dev)
    v = torch.full((N + 1,), SENTINEL, dtype=torch.float64, device=dev)
    work = torch.empty(int(lib.pm_moments_exact_work_len(N, H)), dtype=torch.float64, device=dev)
    rc = lib.pm_moments_exact_lin_f64(_ptr(Yd), ldy, _ptr(mud), _ptr(P), _ptr(G), _ptr(lp), _ptr(vals), K, N, D, H, _ptr(E), lde,
                                      _ptr(C), ldc, _ptr(v), _ptr(work), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    E, C, v = E.cpu().numpy(), C.cpu().numpy(), v.cpu().numpy()
    assert np.all(E[:, H:] == SENTINEL) and np.all(C[:, npair:] == SENTINEL) and v[N] == SENTINEL
    return E[:, :H], C[:, :npair], v[:N]


def _err(got, want):
    scale = np.abs(want).max(axis=1)
    return float((np.abs(got - want).max(axis=1) / np.where(scale > 0, scale, 1.0)).max())


def _check(tag, got, want):
    eE, eC = _err(got[0], want[0]), _err(got[1], want[1])
    ev = float(np.abs(got[2] - want[2]).max() / max(np.abs(want[2]).max(), 1.0))
    print("moments exact ABI %-28s E %.2e  C %.2e  v %.2e (bound %.0e)" % (tag, eE, eC, ev, RTOL))
    assert max(eE, eC, ev) <= RTOL, (tag, eE, eC, ev)


def _bsc(seed, D, H, N, pi=None, sigma=0.9, mu=False):
    rng = np.random.RandomState(seed)
    pi = min(0.4, 2.0 / H) if pi is None else pi
    W = rng.normal(size=(D, H))
    Y = (rng.random_sample((N, H)) < pi) @ W.T + sigma * rng.normal(size=(N, D))
    m = rng.normal(size=D) if mu else None
    if mu:
        Y = Y + m
    return Y, W, sigma, [0., 1.], np.tile(np.log([1 - pi, pi]), (H, 1)), m


# (tag, H, N, D, mu, plan cell [L, CH, chunks, R, pinned sweeps, lo-lo pairs, pair ranges])
CASES = [
    ("H=1: no pair", 1, 4, 5, False, [1, 2, 1, 1, 0, 1, 1]),
    ("H=2: one pair", 2, 4, 5, False, [2, 4, 1, 1, 0, 3, 1]),
    ("H=6 N=5: one chunk, idle lo slots", 6, 5, 7, False, [6, 64, 1, 1, 0, 21, 1]),
    ("H=11: first hi digit", 11, 3, 12, False, [10, 1024, 2, 1, 1, 55, 1]),
    ("H=13 N=67 mu: 8 chunks, R=4", 13, 67, 9, True, [10, 1024, 8, 4, 3, 55, 1]),
    ("H=6 N=300: second row block", 6, 300, 7, False, [6, 64, 1, 1, 0, 21, 1]),
    ("H=15 N=3: two pair ranges", 15, 3, 8, False, [10, 1024, 32, 16, 5, 55, 2]),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_against_enumeration(dev, case):
    tag, H, N, D, mu, cell = case
    p = _plan(N, D, 2, H)
    assert p[2:9] == cell and p[0] == 256 and p[1] == (N + 255) // 256
    args = _bsc(H, D, H, N, mu=mu)
    _check(tag, _run(dev, *args), X.moments(*args))


def test_three_values(dev):
    """K = 3, values {-1, 0, 1}, H = 8: CH = 729 with a ragged last lo state; E[s_h^2] != E[s_h]; chunks of a zero pinned value
    are skipped, those of -1 enter with their sign."""
    H, D, N = 8, 9, 9
    assert _plan(N, D, 3, H)[2:9] == [6, 729, 9, 4, 2, 21, 1]
    rng = np.random.RandomState(5)
    W = rng.normal(size=(D, H))
    values = [-1., 0., 1.]
    logp = np.log(rng.dirichlet([1., 2., 1.], size=H))
    idx = np.array([rng.choice(3, p=np.exp(logp[h]), size=N) for h in range(H)]).T
    Y = np.asarray(values)[idx] @ W.T + 0.8 * rng.normal(size=(N, D))
    got, want = _run(dev, Y, W, 0.8, values, logp), X.moments(Y, W, 0.8, values, logp)
    _check("K=3 H=8", got, want)
    diag = np.cumsum([0] + [H - h for h in range(H - 1)])
    assert np.abs(got[1][:, diag] - got[0]).max() > 1e-3


def test_three_values_ragged_pair_ranges(dev):
    """K = 3, H = 10: 81 chunks in 5 pair ranges of 16 or 17, 40 ranges for E and v; four pinned digits of three values."""
    H, D, N = 10, 8, 4
    assert _plan(N, D, 3, H)[2:9] == [6, 729, 81, 40, 4, 21, 5]
    rng = np.random.RandomState(6)
    W = rng.normal(size=(D, H))
    values = [-1., 0., 1.]
    logp = np.log(rng.dirichlet([1., 2., 1.], size=H))
    Y = rng.normal(size=(N, D)) * 1.5
    _check("K=3 H=10", _run(dev, Y, W, 0.9, values, logp), X.moments(Y, W, 0.9, values, logp))


def test_zero_prior_latents(dev):
    """pi_k = 0 in a lo and in a hi digit: those states carry weight 0, their moments are exactly 0."""
    Y, W, sigma, values, logp, _ = _bsc(7, 9, 12, 6)
    with np.errstate(divide="ignore"):
        logp[3] = np.log([1.0, 0.0])
        logp[11] = np.log([1.0, 0.0])
    assert _plan(6, 9, 2, 12)[2:9] == [10, 1024, 4, 2, 2, 55, 1]
    got, want = _run(dev, Y, W, sigma, values, logp), X.moments(Y, W, sigma, values, logp)
    _check("zero prior", got, want)
    iu = X.pair_index(12)
    dead = (iu[0] == 3) | (iu[1] == 3) | (iu[0] == 11) | (iu[1] == 11)
    assert np.all(got[0][:, [3, 11]] == 0.0) and np.all(got[1][:, dead] == 0.0)


def test_identity_dictionary_every_level(dev):
    """W = c I, D = H = 24, N = 3: 2^14 chunks, R = 256, 14 pinned sweeps -- against the closed form."""
    H, c, pi, sigma = 24, 1.3, 0.2, 0.7
    assert _plan(3, H, 2, H)[2:9] == [10, 1024, 1 << 14, 256, 14, 55, 256]
    rng = np.random.RandomState(2)
    Y = c * (rng.random_sample((3, H)) < pi) + sigma * rng.normal(size=(3, H))
    E, C, v = _run(dev, Y, c * np.eye(H), sigma, [0., 1.], np.tile(np.log([1 - pi, pi]), (H, 1)))
    p, Cc = closed_form(Y, c, pi, sigma)
    a = np.log(pi / (1 - pi)) + (c * Y - 0.5 * c * c) / sigma ** 2
    vv = (H * np.log(1 - pi) + np.logaddexp(0.0, a).sum(axis=1))
    _check("W = c I, H = 24", (E, C, v), (p, Cc, vv))


def test_bits(dev):
    """E is pm_recon_exact_lin_f64's; a NaN row stays alone; the same bits under a row permutation, in a shard, on a second
    call, from the deterministic library and with odd leading dimensions."""
    args = _bsc(13, 9, 13, 67, mu=True)
    Y = args[0].copy()
    E, C, v = _run(dev, *args)
    assert np.array_equal(E, _run(dev, *args, recon=True))
    for other in (_run(dev, *args), _run(dev, *args, det=True), _run(dev, *args, pad=(3, 1, 5))):
        assert all(np.array_equal(a, b) for a, b in zip((E, C, v), other))
    perm = np.random.RandomState(0).permutation(67)
    got = _run(dev, Y[perm], *args[1:])
    assert all(np.array_equal(a[perm], b) for a, b in zip((E, C, v), got))
    got = _run(dev, Y[20:41], *args[1:])
    assert all(np.array_equal(a[20:41], b) for a, b in zip((E, C, v), got))
    Y[5, 2] = np.nan
    got = _run(dev, Y, *args[1:])
    ok = np.arange(67) != 5
    assert all(np.all(np.isnan(g[5])) for g in got)
    assert all(np.array_equal(a[ok], b[ok]) for a, b in zip((E, C, v), got))
    # ... and across the row blocks of the host walk
    args = _bsc(6, 7, 6, 300)
    E, C, v = _run(dev, *args)
    got = _run(dev, args[0][250:], *args[1:])
    assert all(np.array_equal(a[250:], b) for a, b in zip((E, C, v), got))
    assert np.array_equal(E, _run(dev, *args, recon=True))


def test_range_error_needs_no_rows(dev):
    import torch
    from prosper_amd import _lib
    w = torch.empty(4, dtype=torch.float64, device=dev)
    rc = _lib.load().pm_moments_exact_lin_f64(None, 40, None, _ptr(w), _ptr(w), _ptr(w), _ptr(w), 2, 0, 40, 33, None, 33, None,
                                              33 * 17, None, _ptr(w), None)
    assert rc == -2
