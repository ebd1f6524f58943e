"""The C entries of masked_train.hip against NumPy loops: the row statistics to 1e-13 of the largest entry, the
pair tensor BIT FOR BIT (pm_bsc_mtrain_pairs_f64 adds every cell in ascending row order, as the loop does; an entry is
either untouched or one such sum), leading dimensions larger than the rows, the ordered column sums, the solve kernel's pivot
rule, and PM_EINVAL / PM_ERANGE before a device is touched."""
import ctypes

import numpy as np
import pytest

import masked_train_reference as T

pytestmark = pytest.mark.gpu

PM_EINVAL, PM_ERANGE = -1, -2


@pytest.fixture(scope="module")
def lib():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    from prosper_amd import _lib
    return _lib.load()


_KEEP = []


@pytest.fixture(autouse=True)
def _release():
    yield
    del _KEEP[:]


def _dev(a, dtype=None):
    """Device copy of ``a``, kept alive until the test ends (its address is handed to the C entries)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()
    _KEEP.append(t)
    return t


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _rows_problem(rng, N, H, Hp, g):
    SM = T.state_matrix(Hp, g)
    S = SM.shape[0]
    sizes = np.concatenate([[0.0], np.ones(H), SM.sum(axis=1)])
    ppil, ecoef = -1.3, -0.4
    e = rng.uniform(0.5, 30.0, size=(N, 1 + H + S))
    logpj = ppil * sizes[None, :] + ecoef * e
    cand = np.array([rng.permutation(H)[:Hp] for _ in range(N)], dtype=np.int32)
    masks = (SM.astype(np.int64) << np.arange(Hp)[None, :]).sum(axis=1).astype(np.uint16) if S else np.zeros(1, np.uint16)
    return SM, S, logpj, e, cand, masks, ppil, ecoef


@pytest.mark.parametrize("N,H,Hp,g,pad", [(37, 6, 6, 6, 0), (130, 24, 6, 3, 5), (50, 130, 12, 3, 3), (40, 256, 16, 2, 0),
                                          (8269, 8, 5, 3, 1), (20, 3, 1, 1, 2)])
def test_row_statistics(lib, N, H, Hp, g, pad):
    import torch
    from prosper_amd._lib import EStepParams
    rng = np.random.RandomState(N + H)
    SM, S, logpj, e, cand, masks, ppil, ecoef = _rows_problem(rng, N, H, Hp, g)
    K = 1 + H + S
    npair = Hp * (Hp - 1) // 2
    Es, q2, energy, lse = T.row_stats(logpj, e, cand.astype(np.int64), SM, H)
    ldl, lde, ldq = K + pad, H + pad, max(npair, 1) + pad
    lp = torch.full((N, ldl), float("nan"), dtype=torch.float64, device="cuda")
    lp[:, :K] = _dev(logpj)
    es = torch.full((N, lde), -7.0, dtype=torch.float64, device="cuda")
    q2d = torch.full((N, ldq), -7.0, dtype=torch.float64, device="cuda")
    en = torch.empty(N, dtype=torch.float64, device="cuda")
    P = EStepParams(pil_bar=ppil, ecoef=ecoef, prior_scale=1.0, mu_sqnorm=0.0)
    args = [_p(lp), ldl, _p(_dev(lse)), _p(_dev(cand)), _p(_dev(masks.view(np.int16))), S, ctypes.byref(P), N, H, Hp, _p(es), lde,
            _p(q2d), ldq, _p(en), None]
    assert lib.pm_bsc_mtrain_rows_f64(*args) == 0
    torch.cuda.synchronize()
    for name, got, want in (("E[s]", es[:, :H], Es), ("q2", q2d[:, :npair], q2), ("energy", en, energy)):
        got = got.cpu().numpy()
        err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300) if want.size else 0.0
        print("rows N=%d H=%d H'=%d %-6s %.2e" % (N, H, Hp, name, err))
        assert err <= 1e-13, (name, err)
    assert (es[:, H:] == -7.0).all() and (q2d[:, npair:] == -7.0).all()       # the padding of a longer row is not written
    # arguments are checked before a device is touched
    for i, bad in ((0, None), (2, None), (3, None), (10, None), (14, None), (7, -1), (1, K - 1), (11, H - 1)):
        a = list(args)
        a[i] = bad
        assert lib.pm_bsc_mtrain_rows_f64(*a) == PM_EINVAL, i
    if npair:
        a = list(args)
        a[13] = npair - 1
        assert lib.pm_bsc_mtrain_rows_f64(*a) == PM_EINVAL
    a = list(args)
    a[9] = 17
    assert lib.pm_bsc_mtrain_rows_f64(*a) == PM_ERANGE
    a = list(args)
    a[7] = 0
    a[0] = a[2] = None
    assert lib.pm_bsc_mtrain_rows_f64(*a) == PM_EINVAL       # (null pointers are refused at N = 0 too)


@pytest.mark.parametrize("N,D,H,Hp,pad", [(37, 20, 6, 6, 0), (130, 70, 24, 6, 3), (200, 33, 65, 6, 1), (300, 24, 130, 12, 0),
                                          (500, 8, 256, 16, 2), (64, 1024, 10, 5, 0), (40, 64, 4, 3, 0), (90, 65, 16, 4, 5),
                                          (20, 10, 3, 1, 0)])
def test_pair_tensor_bit_for_bit(lib, N, D, H, Hp, pad):
    import torch
    rng = np.random.RandomState(N + D + H)
    npair = Hp * (Hp - 1) // 2
    cand = np.array([rng.permutation(H)[:Hp] for _ in range(N)], dtype=np.int32)
    q2 = rng.uniform(size=(N, npair)) ** 4
    M = rng.uniform(size=(N, D)) < 0.5
    M[0], M[1 % N] = True, False
    diag = rng.uniform(size=(H, D))
    want = T.pair_tensor(cand.astype(np.int64), q2, M, diag.T, H)
    ldq, ldm, ldd = max(npair, 1) + pad, D + pad, D + pad
    q2d = torch.full((N, ldq), float("nan"), dtype=torch.float64, device="cuda")
    q2d[:, :npair] = _dev(q2)
    Md = torch.full((N, ldm), 1, dtype=torch.uint8, device="cuda")
    Md[:, :D] = _dev(M.view(np.uint8)) * 3           # (any non-zero byte means observed)
    dd = torch.full((H, ldd), float("nan"), dtype=torch.float64, device="cuda")
    dd[:, :D] = _dev(diag)
    A = torch.full((D, H, H), float("nan"), dtype=torch.float64, device="cuda")
    args = [_p(_dev(cand)), _p(q2d), ldq, _p(Md), ldm, _p(dd), ldd, N, D, H, Hp, _p(A), None]
    assert lib.pm_bsc_mtrain_pairs_f64(*args) == 0
    torch.cuda.synchronize()
    got = A.cpu().numpy()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), np.abs(got - want).max()
    assert np.array_equal(got, got.transpose(0, 2, 1))
    for i, bad in ((0, None), (3, None), (5, None), (11, None), (7, -1), (4, D - 1), (6, D - 1)):
        a = list(args)
        a[i] = bad
        assert lib.pm_bsc_mtrain_pairs_f64(*a) == PM_EINVAL, i
    if npair:
        for i, bad in ((1, None), (2, npair - 1)):
            a = list(args)
            a[i] = bad
            assert lib.pm_bsc_mtrain_pairs_f64(*a) == PM_EINVAL, i
    for i, bad in ((9, 257), (10, 17), (8, (1 << 28) // (H * H) + 1)):
        a = list(args)
        a[i] = bad
        if i == 8:
            a[4] = a[6] = bad
        assert lib.pm_bsc_mtrain_pairs_f64(*a) == PM_ERANGE, i


def test_pair_tensor_skips_bad_candidates(lib):
    """A candidate outside [0, H) or a pair of equal candidates is skipped, never used as an index."""
    import torch
    N, D, H, Hp = 6, 5, 7, 3
    cand = np.array([[0, 1, 2], [-1, 3, 4], [7, 5, 6], [2, 2, 3], [1 << 20, 0, 1], [4, 5, 6]], dtype=np.int32)
    q2 = np.arange(1, N * 3 + 1, dtype=np.float64).reshape(N, 3)
    A = torch.full((D, H, H), float("nan"), dtype=torch.float64, device="cuda")
    M = torch.ones((N, D), dtype=torch.uint8, device="cuda")
    diag = torch.zeros((H, D), dtype=torch.float64, device="cuda")
    assert lib.pm_bsc_mtrain_pairs_f64(_p(_dev(cand)), _p(_dev(q2)), 3, _p(M), D, _p(diag), D, N, D, H, Hp, _p(A), None) == 0
    torch.cuda.synchronize()
    want = np.zeros((H, H))
    for n in range(N):
        for p, (i, j) in enumerate(T.pair_list(Hp)):
            a, b = cand[n, i], cand[n, j]
            if 0 <= a < H and 0 <= b < H and a != b:
                want[a, b] += q2[n, p]
                want[b, a] += q2[n, p]
    assert np.array_equal(A.cpu().numpy(), np.broadcast_to(want, (D, H, H)))


@pytest.mark.parametrize("N,C,pad", [(1, 1, 0), (37, 6, 2), (8269, 8, 0), (20000, 300, 4), (100000, 1, 0)])
def test_ordered_column_sums(lib, N, C, pad):
    import torch
    rng = np.random.RandomState(N + C)
    X = rng.normal(size=(N, C + pad))
    Xd = _dev(X)
    wl = lib.pm_col_sum_ordered_work_len(N, C)
    work = torch.empty(wl, dtype=torch.float64, device="cuda")
    out = [torch.empty(C, dtype=torch.float64, device="cuda") for _ in range(2)]
    for o in out:
        assert lib.pm_col_sum_ordered_f64(_p(Xd), C + pad, N, C, _p(work), _p(o), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[0], out[1])
    want = X[:, :C].sum(axis=0)
    # (a sum of N terms in another order: N eps of the sum of magnitudes)
    assert (np.abs(out[0].cpu().numpy() - want) <= N * 2.3e-16 * np.abs(X[:, :C]).sum(axis=0)).all()
    assert lib.pm_col_sum_ordered_f64(None, C, N, C, _p(work), _p(out[0]), None) == PM_EINVAL
    assert lib.pm_col_sum_ordered_f64(_p(Xd), C - 1, N, C, _p(work), _p(out[0]), None) == PM_EINVAL
    assert lib.pm_col_sum_ordered_f64(_p(Xd), C, -1, C, _p(work), _p(out[0]), None) == PM_EINVAL
    assert lib.pm_col_sum_ordered_work_len(-1, C) == -1


@pytest.mark.parametrize("D,H", [(5, 6), (3, 65), (2, 256)])
def test_solve_and_the_pivot_rule(lib, D, H):
    import torch
    rng = np.random.RandomState(D + H)
    Q = rng.normal(size=(D, H, H))
    A = Q @ Q.transpose(0, 2, 1) + 0.5 * np.eye(H)[None]
    Ainv = np.linalg.inv(A)
    Ainv = 0.5 * (Ainv + Ainv.transpose(0, 2, 1))
    r = rng.normal(size=(H, D + 2))
    Wold = rng.normal(size=(H, D + 1))
    piv = np.tile([1.0, 2.0], (D, 1))
    piv[0] = [0.0, 1.0]                      # not positive
    if D > 2:
        piv[2] = [1e-12, 1.0]                # ratio below 1e-11
    Wnew = torch.full((H, D + 3), -7.0, dtype=torch.float64, device="cuda")
    status = torch.full((D,), 9, dtype=torch.int32, device="cuda")
    args = [_p(_dev(A)), _p(_dev(Ainv)), _p(_dev(piv)), _p(_dev(r)), D + 2, _p(_dev(Wold)), D + 1, D, H, _p(Wnew), D + 3,
            _p(status), None]
    assert lib.pm_bsc_mtrain_solve_f64(*args) == 0
    torch.cuda.synchronize()
    got, st = Wnew.cpu().numpy(), status.cpu().numpy()
    kept = [0] + ([2] if D > 2 else [])
    assert list(np.nonzero(st == 0)[0]) == kept and set(st) <= {0, 1}
    for d in range(D):
        if d in kept:
            assert np.array_equal(got[:, d], Wold[:, d])
        else:
            want = np.linalg.solve(A[d], r[:, d])
            assert np.abs(got[:, d] - want).max() <= 1e-10 * np.abs(want).max()
    assert (got[:, D:] == -7.0).all()
    for i, bad in ((0, None), (1, None), (2, None), (3, None), (5, None), (9, None), (11, None), (4, D - 1), (6, D - 1),
                   (10, D - 1), (7, 0)):
        a = list(args)
        a[i] = bad
        assert lib.pm_bsc_mtrain_solve_f64(*a) == PM_EINVAL, i
    a = list(args)
    a[8] = 257
    assert lib.pm_bsc_mtrain_solve_f64(*a) == PM_ERANGE
