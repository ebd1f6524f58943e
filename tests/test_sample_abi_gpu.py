"""The pm_sample_* entries through the C ABI against tests/sample_reference.py: indices exactly, lists exactly,
decoded rows to the project's 1e-11 row-relative bound, one case per instantiation and branch (table in DESIGN 4.20).

Indices.  U is drawn on the host from a seeded RandomState; every u within 1e-9 c_{K-1} of a CDF edge of the reference is first
moved to the middle of its interval (sample_reference.nudge: the cap -- the two sides build the CDF in different orders and
their exp differ in the last bit, so a u closer to an edge than the CDF's rounding error, ~K 2^-53 c_{K-1} < 1e-12 c_{K-1} at
K = 1200, could fall either way); no draw is left out, and then idx equals the reference's in every entry."""
import ctypes

import numpy as np
import pytest

import recon_reference as R
import sample_reference as SR

pytestmark = pytest.mark.gpu

RTOL = 1e-11
TINY = np.finfo(np.float64).tiny


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _t(dev, a, dtype=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _states(dev, lp, U, a=1.0, off=None, floor=0.0, null=-1, lse=None, ld=None, ldu=None, det=False):
    """pm_sample_states_f64 on host arrays (leading dimensions padded with NaN when asked): idx (N, M) int32."""
    import torch
    from prosper_amd import _lib
    N, K = lp.shape
    M = U.shape[1]
    ld, ldu = ld or K, ldu or M
    X = np.full((N, ld), np.nan)
    X[:, :K] = lp
    Up = np.full((N, ldu), np.nan)
    Up[:, :M] = U
    Xd, Ud = _t(dev, X), _t(dev, Up)
    od = _t(dev, off) if off is not None else None
    ld_ = _t(dev, lse) if lse is not None else None
    idx = torch.full((N, M), -7, dtype=torch.int32, device=dev)
    _lib.call("pm_sample_states_f64", _p(Xd), ld, _p(ld_), ctypes.c_double(a), _p(od), ctypes.c_double(floor), null, _p(Ud),
              ldu, N, K, M, _p(idx), None, det=det)
    torch.cuda.synchronize()
    return idx.cpu().numpy()


# K: within one 64-column chunk, exactly one, several with a ragged last one (1 + 24 + C(6,2) + C(6,3) = 60 ... the E-steps'
# 1 + H + S), seg = 3, 5 and 19 columns per lane, and past 1984 columns (three wavefronts per workgroup instead of four)
@pytest.mark.parametrize("K,M", [(1, 3), (9, 1), (60, 64), (64, 65), (65, 5), (130, 64), (167, 65), (311, 7), (1199, 65),
                                 (2100, 3)])
def test_indices_are_exact(dev, K, M):
    rng = np.random.RandomState(K + M)
    N = 23
    lp = rng.normal(size=(N, K)) * 3
    lp[rng.uniform(size=lp.shape) < 0.05] = -np.inf              # columns of weight exactly 0
    lp[:, 0] = np.where(np.isinf(lp).all(axis=1), 0.0, lp[:, 0])
    U, moved = SR.nudge(rng.uniform(size=(N, M)), SR.cdfs(lp))
    want = SR.draw_states(lp, U)
    got = _states(dev, lp, U, ld=K + 3, ldu=M + 2)
    print("states K=%d M=%d: %d of %d uniforms moved off an edge" % (K, M, moved, U.size))
    assert np.array_equal(got, want)
    assert np.array_equal(_states(dev, lp, U, det=True), want)
    w = SR.weights(lp)
    assert (np.take_along_axis(w, got.astype(np.int64), 1) > 0).all()


def test_scale_offsets_floor_and_given_normaliser(dev):
    rng = np.random.RandomState(5)
    N, K, M = 17, 75, 33
    lp, off = rng.normal(size=(N, K)) * 4, rng.normal(size=K)
    U = rng.uniform(size=(N, M))
    U1, _ = SR.nudge(U, SR.cdfs(lp, a=-0.5, off=off))
    assert np.array_equal(_states(dev, lp, U1, a=-0.5, off=off), SR.draw_states(lp, U1, a=-0.5, off=off))
    # GSC's weights: exp(lp / 2) against a normaliser of zeros, floored at DBL_MIN everywhere but in the null column
    lp2 = lp.copy()
    lp2[:, 3] = -4000.0                       # underflows: the floor gives it weight DBL_MIN, reachable only at u ~ 0
    lp2[2, :] = -4000.0                       # a row whose weights all underflow: null column 0, the others DBL_MIN each
    kw = dict(SR.GSC_WEIGHTS, lse=np.zeros(N))
    U2, _ = SR.nudge(U, SR.cdfs(lp2, **kw))
    got = _states(dev, lp2, U2, a=0.5, floor=TINY, null=0, lse=np.zeros(N))
    assert np.array_equal(got, SR.draw_states(lp2, U2, **kw))
    assert (got[2] >= 1).all()                # (the null state of that row has weight exactly 0)


def test_every_state_is_reachable_and_the_edges(dev):
    K = 11
    w = np.array([0., 3., 1., 0., 0., 2., 5., 0., 1., 4., 0.])
    with np.errstate(divide="ignore"):
        lp = np.log(w)[None, :].repeat(3, axis=0)
    lp[1] = lp[1] + 700.0                      # the same weights far from 1: the row's log-sum-exp takes it out
    lp[2, 4] = np.nan
    c = np.cumsum(w) / w.sum()
    pos = np.nonzero(w)[0]
    mids = np.array([0.5 * (c[k] + (c[k - 1] if k else 0.0)) for k in pos])
    U = np.concatenate([mids, [0.0, SR.U_MAX, -1.0, 1.0, 2.5, np.nan, -np.inf, np.inf]])[None, :].repeat(3, axis=0)
    got = _states(dev, lp, U)
    want = list(pos) + [pos[0], pos[-1], pos[0], pos[-1], pos[-1], pos[0], pos[0], pos[-1]]
    assert got[0].tolist() == want and got[1].tolist() == want
    assert (got[2] == -1).all()
    # all weight in one column; a row of -inf has no draw
    lp = np.full((2, 70), -np.inf)
    lp[0, 69] = 2.0
    got = _states(dev, lp, np.array([[0.0, 0.3, SR.U_MAX]] * 2))
    assert got[0].tolist() == [69, 69, 69] and got[1].tolist() == [-1, -1, -1]


def _active(dev, idx, cand, H, blocks, soff, moff, table, A, K):
    import torch
    from prosper_amd import _lib
    N, M = idx.shape
    S = 0 if table is None else len(table)
    Hp = cand.shape[1] if S else 0
    ai = torch.full((N, M, A), -9, dtype=torch.int32, device=dev)
    av = torch.full((N, M, A), 77.0, dtype=torch.float64, device=dev)
    bv = (ctypes.c_double * 8)(*(list(blocks) + [0.0] * (8 - len(blocks))))
    idx_d = _t(dev, idx, np.int32)
    cd = _t(dev, cand, np.int32) if S else None
    td = _t(dev, table, np.float64) if S else None
    _lib.call("pm_sample_active_f64", _p(idx_d), _p(cd), _p(td), bv, N, M, H, Hp, K, soff, len(blocks), moff, S, A, _p(ai),
              _p(av), None)
    torch.cuda.synchronize()
    return ai, av


def _decode_lin(dev, ai, av, W, mu, lay="mnd", ldw=None):
    import torch
    from prosper_amd import _lib
    N, M, A = ai.shape
    D, H = W.shape
    ldw = ldw or D
    Wt = np.full((H, ldw), np.nan)
    Wt[:, :D] = W.T
    Wd = _t(dev, Wt)
    mud = _t(dev, mu) if mu is not None else None
    if lay == "mnd":
        out = torch.full((M, N, D), 55.0, dtype=torch.float64, device=dev)
        ldn, ldm = D, N * D
    else:                                     # (N, M, D + 3): the other order, padded rows
        out = torch.full((N, M, D + 3), 55.0, dtype=torch.float64, device=dev)
        ldn, ldm = M * (D + 3), D + 3
    _lib.call("pm_sample_decode_lin_f64", _p(ai), _p(av), A, _p(Wd), ldw, _p(mud), N, M, H, D, _p(out), ldn, ldm, None)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    if lay != "mnd":
        assert (o[:, :, D:] == 55.0).all()
        o = o[:, :, :D].transpose(1, 0, 2)
    return o


def _rel(got, want):
    M, N, D = want.shape
    return R.row_rel_err(got.reshape(M * N, D), want.reshape(M * N, D))


# (layout, D, H, Hp, table kind): BSC-like binary table, DSC with 7 value blocks, TSC with a latent held twice, a mixture (S = 0)
@pytest.mark.parametrize("kind,D,H,Hp,g", [("bsc", 1, 6, 4, 2), ("bsc", 64, 24, 6, 3), ("bsc", 65, 130, 12, 3), ("bsc", 1024, 8, 5, 5),
                                           ("bsc", 9, 40, 16, 2), ("dsc8", 12, 9, 4, 3), ("tsc", 10, 70, 4, 4),
                                           ("mix", 33, 21, 1, 1)])
def test_active_list_and_linear_decode(dev, kind, D, H, Hp, g):
    import itertools
    from prosper_amd.em.camodels import generate_state_matrix
    rng = np.random.RandomState(D + H)
    N, M = 19, 5
    SM = generate_state_matrix(Hp, g)[2].astype(np.float64) if kind != "mix" else None
    cand = np.array([np.sort(rng.permutation(H)[:Hp]) for _ in range(N)])
    mu = rng.normal(size=D) if kind == "bsc" else None
    if kind == "bsc":
        blocks, soff, moff, table = (1.0,), 1, 1 + H, SM
    elif kind == "dsc8":
        blocks, soff, moff = (-3., -2., -1., 1., 2., 3., 4.), 1, 1 + 7 * H
        table = SM * rng.choice(blocks, size=SM.shape)
    elif kind == "tsc":
        blocks, soff, moff = (), 0, 0
        table = np.array(list(itertools.product([-1., 0., 1.], repeat=Hp)))
        cand[::3, 2] = cand[::3, 0]
    else:
        blocks, soff, moff, table = (1.0,), 0, 0, None
    S = 0 if table is None else len(table)
    K = max(moff + S, soff + len(blocks) * H)
    A = max(1, int((table != 0).sum(1).max())) if S else 1
    idx = rng.randint(0, K, size=(N, M)).astype(np.int32)
    idx[0, :3] = [0, K - 1, soff]
    idx[4, :] = -1
    W = rng.normal(size=(D, H))
    ai, av = _active(dev, idx, cand, H, blocks, soff, moff, table, A, K)
    wi, wv = SR.active_list(idx, cand, H, blocks, soff, moff, table, A)
    assert np.array_equal(ai.cpu().numpy(), wi)
    assert np.array_equal(av.cpu().numpy(), wv, equal_nan=True)
    want = SR.decode_linear(wi, wv, W, mu)
    keep = np.ones(N, dtype=bool)
    keep[4] = False
    for lay, ldw in (("mnd", None), ("nmd", D + 5)):
        got = _decode_lin(dev, ai, av, W, mu, lay, ldw)
        assert np.isnan(got[:, 4]).all()
        err = _rel(got[:, keep], want[:, keep])
        print("decode_lin %s D=%d H=%d A=%d %s: row-relative error %.3e" % (kind, D, H, A, lay, err))
        assert err <= RTOL
    S_want = SR.latents_from_active(wi, wv, H)
    from prosper_amd.em.camodels._device import DeviceCAModel
    S_got = DeviceCAModel._sample_scatter(_t(dev, idx, np.int32), ai, av, H).cpu().numpy()
    assert np.array_equal(S_got, S_want, equal_nan=True)


@pytest.mark.parametrize("signed,rho", [(False, 21.0), (True, 6.0), (False, 9.5), (True, 9.5)])
@pytest.mark.parametrize("D,H,Hp,g", [(1, 6, 4, 2), (64, 24, 6, 3), (65, 12, 5, 3), (1024, 24, 16, 2)])
def test_mca_decode(dev, signed, rho, D, H, Hp, g):
    import torch
    from prosper_amd import _lib
    from prosper_amd.em.camodels import generate_state_matrix
    rng = np.random.RandomState(D + H + int(rho))
    N, M = 11, 4
    SM = generate_state_matrix(Hp, g)[2]
    S = len(SM)
    masks = (SM.astype(np.int64) << np.arange(Hp)[None, :]).sum(axis=1).astype(np.uint16)
    cand = np.array([rng.permutation(H)[:Hp] for _ in range(N)])
    W = rng.uniform(-2, 3, size=(D, H)) if signed else rng.uniform(0.1, 3, size=(D, H))
    W = np.where(np.abs(W) < 0.05, 0.05, W)
    Wrho = (np.sign(W) * np.abs(W) ** rho).T if signed else (W ** rho).T
    K = 1 + H + S
    idx = rng.randint(0, K, size=(N, M)).astype(np.int32)
    idx[0, :3] = [0, 1, K - 1]
    idx[3, 1] = -1
    out = torch.full((M, N, D), 55.0, dtype=torch.float64, device=dev)
    args = [_t(dev, idx, np.int32), _t(dev, cand, np.int32), _t(dev, masks.view(np.int16)), _t(dev, W.T.copy()), _t(dev, Wrho)]
    _lib.call("pm_sample_decode_mca_f64", *[_p(t) for t in args], ctypes.c_double(1. / rho), int(signed), N, M, H, D, Hp, S,
              _p(out), D, N * D, None)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    want = SR.decode_mca(idx, cand, SM, W, rho, signed)
    assert np.isnan(got[1, 3]).all() and np.isnan(want[1, 3]).all()
    got[1, 3] = want[1, 3] = 0.0
    err = _rel(got, want)
    print("decode_mca signed=%d rho=%g D=%d H'=%d: row-relative error %.3e" % (signed, rho, D, Hp, err))
    assert err <= RTOL
    assert np.array_equal(got[idx.T == 0], np.zeros_like(got[idx.T == 0]))


def _gsc_problem(rng, D, H, N):
    Q = rng.normal(size=(H, H)) * 0.2
    p = {"W": rng.normal(size=(D, H)), "pi": np.full(H, 0.2), "mu": rng.normal(size=H),
         "psi_sq": np.diag(rng.uniform(0.5, 1.5, size=H)) + Q @ Q.T, "sigma_sq": np.float64(0.6)}
    return p, rng.normal(size=(N, D)) * 1.5


@pytest.mark.parametrize("gamma", [2, 3, 4, 6, 8])
def test_gsc_values(dev, gamma):
    """z = kappa_s + L eps at H' = gamma against NumPy (inverse and Cholesky from LAPACK): the lists' latents exactly, the
    values to 1e-11 of the row's largest |z|."""
    import torch
    from prosper_amd import _lib
    from prosper_amd.em.camodels import generate_state_matrix
    rng = np.random.RandomState(gamma)
    D, H, N, M, Hp = 14, 11, 9, 6, gamma
    p, Y = _gsc_problem(rng, D, H, N)
    SM = generate_state_matrix(Hp, gamma)[2]
    S = len(SM)
    masks = (SM.astype(np.int64) << np.arange(Hp)[None, :]).sum(axis=1).astype(np.uint16)
    cand = np.array([np.sort(rng.permutation(H)[:Hp]) for _ in range(N)])
    K = 1 + H + S
    idx = rng.randint(0, K, size=(N, M)).astype(np.int32)
    idx[0, :4] = [0, 1, H, K - 1]                   # null, first and last singleton, the state with every candidate on
    idx[2, 3] = -1
    E = rng.normal(size=(N, M, gamma + 1))           # (a padded leading dimension)
    s2 = 0.6
    W, mu, psi = p["W"], p["mu"], p["psi_sq"]
    Gd = (W * W).sum(axis=0)
    lam = Gd / s2 + 1. / np.diag(psi)
    tables = np.stack([np.zeros(H), 2. * mu / s2, Gd * mu, 1. / (lam * s2 * s2), 1. / (lam * s2), 1. / lam, mu, np.zeros(H)])
    A = gamma
    ai = torch.full((N, M, A), -9, dtype=torch.int32, device=dev)
    av = torch.full((N, M, A), 77.0, dtype=torch.float64, device=dev)
    args = dict(idx=_t(dev, idx, np.int32), cand=_t(dev, cand, np.int32), masks=_t(dev, masks.view(np.int16)),
                sc=_t(dev, Y @ W), G=_t(dev, W.T @ W), psi=_t(dev, psi), tab=_t(dev, tables), E=_t(dev, E))
    _lib.call("pm_sample_gsc_f64", _p(args["idx"]), _p(args["cand"]), _p(args["masks"]), _p(args["sc"]), H, _p(args["G"]),
              _p(args["psi"]), _p(args["tab"]), ctypes.c_double(s2), _p(args["E"]), gamma + 1, N, M, H, Hp, S, gamma, A, _p(ai),
              _p(av), None)
    torch.cuda.synchronize()
    wi, wv = SR.gsc_active_list(idx, cand, SM, p, Y, E, A)
    gi, gv = ai.cpu().numpy(), av.cpu().numpy()
    assert np.array_equal(gi, wi)
    assert np.isnan(gv[2, 3]).all()
    gv[2, 3] = wv[2, 3] = 0.0
    err = R.row_rel_err(gv.reshape(N * M, A), wv.reshape(N * M, A))
    print("sample_gsc gamma=%d: row-relative error of z %.3e" % (gamma, err))
    assert err <= RTOL
    # psi_sq that is not positive definite on a state's candidates: NaN values for that state, none elsewhere
    bad = psi.copy()
    h0 = int(cand[0, 0])
    bad[h0, h0] = -1.0
    _lib.call("pm_sample_gsc_f64", _p(args["idx"]), _p(args["cand"]), _p(args["masks"]), _p(args["sc"]), H, _p(args["G"]),
              _p(_t(dev, bad)), _p(args["tab"]), ctypes.c_double(s2), _p(args["E"]), gamma + 1, N, M, H, Hp, S, gamma, A, _p(ai),
              _p(av), None)
    torch.cuda.synchronize()
    assert np.isnan(av[0, 3].cpu().numpy()).all() and np.isfinite(av[0, 1].cpu().numpy()).all()


def test_second_trip_of_every_row_loop(dev):
    """N = 8269: the state kernel walks 8192 rows per trip (2048 workgroups of four wavefronts), the list kernels 524288
    (row, sample) pairs (M = 64: 529216), the decode kernels 32768 pairs (M = 4: 33076).  The rows from 150 before the
    boundary to the end against NumPy; everything bit for bit against 4096-row shards given the matching rows of U."""
    rng = np.random.RandomState(8269)
    N, K, M, H, D = 8269, 9, 64, 6, 5
    lp = rng.normal(size=(N, K)) * 2
    U, _ = SR.nudge(rng.uniform(size=(N, M)), SR.cdfs(lp))
    idx = _states(dev, lp, U)
    tail = slice(8192 - 150, N)
    assert np.array_equal(idx[tail], SR.draw_states(lp[tail], U[tail]))
    parts = [_states(dev, lp[i:i + 4096], U[i:i + 4096]) for i in range(0, N, 4096)]
    assert np.array_equal(np.concatenate(parts), idx)
    table = np.array([[1., 1.], [1., 0.]])
    cand = rng.randint(0, H, size=(N, 2))
    ai, av = _active(dev, idx, cand, H, (1.0,), 1, 1 + H, table, 2, K)
    t2 = slice(N - 40, N)                          # pairs past 524288 start at row 8192
    wi, wv = SR.active_list(idx[t2], cand[t2], H, (1.0,), 1, 1 + H, table, 2)
    assert np.array_equal(ai.cpu().numpy()[t2], wi) and np.array_equal(av.cpu().numpy()[t2], wv)
    W = rng.normal(size=(D, H))
    got = _decode_lin(dev, ai[:, :4].contiguous(), av[:, :4].contiguous(), W, None)
    want = SR.decode_linear(wi[:, :4], wv[:, :4], W)
    assert _rel(got[:, t2], want) <= RTOL
    sh = np.concatenate([_decode_lin(dev, ai[i:i + 4096, :4].contiguous(), av[i:i + 4096, :4].contiguous(), W, None)
                         for i in range(0, N, 4096)], axis=1)
    assert np.array_equal(sh.view(np.uint64), got.view(np.uint64))


def test_second_trip_of_the_gsc_list_kernel(dev):
    """N = 8269, M = 64: 529216 (row, sample) pairs, 524288 per trip of sample_gsc_kernel.  The last 30 rows against NumPy; the
    whole result bit for bit against 4096-row shards."""
    import torch
    from prosper_amd import _lib
    from prosper_amd.em.camodels import generate_state_matrix
    rng = np.random.RandomState(77)
    N, M, D, H, Hp, gamma = 8269, 64, 7, 6, 3, 2
    p, Y = _gsc_problem(rng, D, H, N)
    SM = generate_state_matrix(Hp, gamma)[2]
    S = len(SM)
    masks = (SM.astype(np.int64) << np.arange(Hp)[None, :]).sum(axis=1).astype(np.uint16)
    cand = np.sort(np.argsort(rng.uniform(size=(N, H)), axis=1)[:, :Hp], axis=1)
    idx = rng.randint(0, 1 + H + S, size=(N, M)).astype(np.int32)
    E = rng.normal(size=(N, M, gamma))
    s2 = 0.6
    W, mu, psi = p["W"], p["mu"], p["psi_sq"]
    Gd = (W * W).sum(axis=0)
    lam = Gd / s2 + 1. / np.diag(psi)
    tables = np.stack([np.zeros(H), 2. * mu / s2, Gd * mu, 1. / (lam * s2 * s2), 1. / (lam * s2), 1. / lam, mu, np.zeros(H)])
    fixed = [_t(dev, masks.view(np.int16)), _t(dev, W.T @ W), _t(dev, psi), _t(dev, tables)]

    def run(sl):
        n = len(idx[sl])
        ai = torch.full((n, M, gamma), -9, dtype=torch.int32, device=dev)
        av = torch.full((n, M, gamma), 77.0, dtype=torch.float64, device=dev)
        part = [_t(dev, idx[sl], np.int32), _t(dev, cand[sl], np.int32), _t(dev, Y[sl] @ W), _t(dev, E[sl])]
        _lib.call("pm_sample_gsc_f64", _p(part[0]), _p(part[1]), _p(fixed[0]), _p(part[2]), H, _p(fixed[1]), _p(fixed[2]),
                  _p(fixed[3]), ctypes.c_double(s2), _p(part[3]), gamma, n, M, H, Hp, S, gamma, gamma, _p(ai), _p(av), None)
        torch.cuda.synchronize()
        return ai.cpu().numpy(), av.cpu().numpy()
    gi, gv = run(slice(0, N))
    tail = slice(N - 30, N)
    wi, wv = SR.gsc_active_list(idx[tail], cand[tail], SM, p, Y[tail], E[tail], gamma)
    assert np.array_equal(gi[tail], wi)
    assert R.row_rel_err(gv[tail].reshape(-1, gamma), wv.reshape(-1, gamma)) <= RTOL
    parts = [run(slice(i, min(i + 4096, N))) for i in range(0, N, 4096)]
    assert np.array_equal(np.concatenate([q[0] for q in parts]), gi)
    assert np.array_equal(np.concatenate([q[1] for q in parts]).view(np.uint64), gv.view(np.uint64))
