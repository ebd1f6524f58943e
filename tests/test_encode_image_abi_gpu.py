"""pm_codes_pool_f64 / pm_codes_pool_finish_f64 through the C ABI, bit for bit against the plain-Python
statement of the summation order (tests/encode_image_reference.py, pinned on the CPU by tests/test_encode_image_cpu.py, which
also shows that the inputs used here make the order visible): every shape class, a leading dimension, every way of cutting
the matrix into ranges of whole patch rows, the maximum's NaN / -inf / tie rules, the division in place, n = 0, both builds.

Shapes (B, nr, nc, gh, gw, H): H in {1, 3, 64, 65, 130} (below, at and past one wavefront of h), nc in {1, 2, 7, 64, 65, 129},
nr in {1, 2, 5}, B in {1, 2, 3}, gw in {1, 2, nc}, gh in {1, 2, nr} -- a covering subset of the product."""
import ctypes as C
import functools

import numpy as np
import pytest

import encode_image_reference as E

pytestmark = pytest.mark.gpu

CASES = [(2, 5, 7, 2, 2, 3), (3, 2, 65, 2, 1, 65), (1, 5, 129, 5, 2, 130), (1, 1, 1, 1, 1, 1), (1, 2, 2, 1, 2, 64),
         (3, 5, 64, 5, 64, 1), (1, 1, 129, 1, 129, 3), (2, 2, 7, 2, 7, 65), (1, 5, 65, 2, 2, 64), (3, 1, 2, 1, 1, 130),
         (1, 2, 64, 1, 2, 130), (1, 5, 7, 1, 1, 64), (3, 5, 1, 2, 1, 3)]
PAD = 3                                                       # ldc = H + PAD, the padding holding NaN


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _problem(case):
    """(codes (N, H), reference sum, reference max): computed once per shape and shared by every test below."""
    B, nr, nc, gh, gw, H = case
    x = E.wide_range(np.random.RandomState(0), (B * nr * nc, H))
    x.setflags(write=False)
    return x, E.pool(x, (B, nr, nc), (gh, gw), "sum"), E.pool(x, (B, nr, nc), (gh, gw), "max")


def _splits(case):
    """Cuts of the B nr patch rows into ascending ranges: the whole matrix; one patch row per call; an uneven split whose
    boundary falls inside a region; one whose middle range spans the end of image b and the start of image b + 1."""
    B, nr, nc, gh, gw, H = case
    rows = B * nr
    out = {"whole": [0, rows], "each row": list(range(rows + 1))}
    inside = [r0 + 1 for r0, r1 in E.pool_regions(nr, gh) if r1 - r0 >= 2]
    if inside:
        out["inside a region"] = sorted(set([0, inside[-1], rows]))
    if B > 1:
        out["across two images"] = sorted(set([0, max(nr - 1, 0), min(nr + 1, rows), rows]))
    return out


def _run(lib, dev, x, case, mode, cuts, acc=None, ld_pad=PAD):
    """The entry over the ranges ``cuts`` describes, from a matrix with leading dimension H + ld_pad; the running result."""
    import torch
    B, nr, nc, gh, gw, H = case
    N = B * nr * nc
    wide = torch.full((N, H + ld_pad), float("nan"), dtype=torch.float64, device=dev)
    wide[:, :H] = torch.from_numpy(np.array(x, dtype=np.float64)).to(dev)       # (a copy: the shared problem is read-only)
    if acc is None:
        acc = torch.full((B, gh, gw, H), float("-inf") if mode else 0.0, dtype=torch.float64, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    for a, b in zip(cuts, cuts[1:]):
        n0, n = a * nc, (b - a) * nc
        need = lib.pm_codes_pool_work_len(n, nc, gw, H)
        assert need == (b - a) * gw * H
        work = torch.full((need + 5,), float("nan"), dtype=torch.float64, device=dev)       # every partial read is written first
        first = wide[n0:] if n0 < N else wide[N - 1:]
        st = lib.pm_codes_pool_f64(C.c_void_p(first.data_ptr()), H + ld_pad, n0, n, B, nr, nc, gh, gw, H, mode,
                                   C.c_void_p(acc.data_ptr()), C.c_void_p(work.data_ptr()), stream)
        assert st == 0, (st, a, b)
        assert bool(torch.isnan(work[need:]).all()), "the scratch was written past its length"
    torch.cuda.synchronize()
    return acc


@pytest.mark.parametrize("det", [False, True], ids=["default", "deterministic"])
@pytest.mark.parametrize("case", CASES)
def test_sum_and_max_equal_the_reference_for_every_split_in_both_builds(dev, case, det):
    from prosper_amd import _lib
    lib = _lib.load(det)
    x, want_sum, want_max = _problem(case)
    for name, cuts in _splits(case).items():
        E.same_bits(_run(lib, dev, x, case, 0, cuts).cpu().numpy(), want_sum, "sum %r %s" % (case, name))
        E.same_bits(_run(lib, dev, x, case, 1, cuts).cpu().numpy(), want_max, "max %r %s" % (case, name))
    E.same_bits(_run(lib, dev, x, case, 0, [0, case[0] * case[1]], ld_pad=0).cpu().numpy(), want_sum, "ldc = H")


@pytest.mark.parametrize("case", CASES)
def test_finish_divides_once_also_in_place(dev, case):
    import torch
    from prosper_amd import _lib
    lib = _lib.load()
    B, nr, nc, gh, gw, H = case
    x, want_sum, _ = _problem(case)
    want = E.pool(x, (B, nr, nc), (gh, gw), "mean")
    acc = _run(lib, dev, x, case, 0, [0, B * nr])
    out = torch.full_like(acc, float("nan"))
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    assert lib.pm_codes_pool_finish_f64(C.c_void_p(acc.data_ptr()), C.c_void_p(out.data_ptr()), B, nr, nc, gh, gw, H, stream) == 0
    E.same_bits(out.cpu().numpy(), want, "mean %r" % (case,))
    E.same_bits(acc.cpu().numpy(), want_sum, "the running sum is left alone")
    assert lib.pm_codes_pool_finish_f64(C.c_void_p(acc.data_ptr()), C.c_void_p(acc.data_ptr()), B, nr, nc, gh, gw, H, stream) == 0
    E.same_bits(acc.cpu().numpy(), want, "mean in place %r" % (case,))


@pytest.mark.parametrize("case", [(2, 5, 7, 2, 2, 3), (1, 5, 65, 2, 2, 64), (3, 2, 65, 2, 1, 65), (2, 2, 7, 2, 7, 65)])
def test_maximum_nan_infinities_and_ties(dev, case):
    from prosper_amd import _lib
    lib = _lib.load()
    B, nr, nc, gh, gw, H = case
    N = B * nr * nc
    rng = np.random.RandomState(5)
    splits = _splits(case)
    # a NaN makes exactly its output NaN -- in the sum as well
    x = _problem(case)[0].copy()
    k, h = N // 2 + 1, H - 1
    x[k, h] = np.nan
    b, rest = divmod(k, nr * nc)
    r, c = divmod(rest, nc)
    i = [n for n, (a, z) in enumerate(E.pool_regions(nr, gh)) if a <= r < z][0]
    j = [n for n, (a, z) in enumerate(E.pool_regions(nc, gw)) if a <= c < z][0]
    hit = np.zeros((B, gh, gw, H), dtype=bool)
    hit[b, i, j, h] = True
    for mode, what in ((1, "max"), (0, "sum")):
        for name, cuts in splits.items():
            got = _run(lib, dev, x, case, mode, cuts).cpu().numpy()
            assert np.array_equal(np.isnan(got), hit), (what, name, np.argwhere(np.isnan(got)))
            E.same_bits(got, E.pool(x, (B, nr, nc), (gh, gw), what), "%s with a NaN, %s" % (what, name))
    # a NaN first or last in its region: no later or earlier compare drops it
    for kk in (0, N - 1):
        x = _problem(case)[0].copy()
        x[kk, 0] = np.nan
        got = _run(lib, dev, x, case, 1, splits["each row"]).cpu().numpy()
        assert np.isnan(got).sum() == 1 and np.isnan(got[0 if kk == 0 else B - 1, 0 if kk == 0 else gh - 1,
                                                         0 if kk == 0 else gw - 1, 0])
    # all -inf stays -inf; +inf wins; a region of -inf and one finite value gives that value
    x = np.full((N, H), -np.inf)
    E.same_bits(_run(lib, dev, x, case, 1, splits["whole"]).cpu().numpy(), np.full((B, gh, gw, H), -np.inf), "all -inf")
    x[::3, 0] = -1e308
    x[1, H - 1] = np.inf
    E.same_bits(_run(lib, dev, x, case, 1, splits["each row"]).cpu().numpy(), E.pool(x, (B, nr, nc), (gh, gw), "max"), "infinities")
    # ties: few distinct values, many repeats; zeros of both signs -- max(-0, +0) = +0 whichever comes first
    x = rng.randint(-2, 3, size=(N, H)).astype(np.float64)
    x[x == 0] = np.where(rng.uniform(size=(x == 0).sum()) < 0.5, 0.0, -0.0)
    x[:, 0] = -0.0
    x[N - 1, 0] = 0.0
    if H > 1:
        x[:, 1] = -0.0
    want = E.pool(x, (B, nr, nc), (gh, gw), "max")
    assert np.signbit(want).any() and (want == 0).any()
    for name, cuts in splits.items():
        E.same_bits(_run(lib, dev, x, case, 1, cuts).cpu().numpy(), want, "ties, %s" % name)


def test_no_rows_leave_the_running_result_as_it_is(dev):
    import torch
    from prosper_amd import _lib
    case = (2, 5, 7, 2, 2, 3)
    B, nr, nc, gh, gw, H = case
    x = _problem(case)[0]
    for det in (False, True):
        lib = _lib.load(det)
        for mode in (0, 1):
            before = torch.from_numpy(E.wide_range(np.random.RandomState(9), (B, gh, gw, H))).to(dev)
            keep = before.clone()
            for R in (0, 3, B * nr):
                _run(lib, dev, x, case, mode, [R, R], acc=before)
            E.same_bits(before.cpu().numpy(), keep.cpu().numpy(), "n = 0")


def test_a_running_result_carries_across_calls(dev):
    """A sum that does not start at +0: the entry adds onto what the caller left (the contract of a running result), so a
    second pass over the same rows doubles nothing silently -- it continues the chain from the first pass's bits."""
    from prosper_amd import _lib
    lib = _lib.load()
    case = (2, 5, 7, 2, 2, 3)
    B, nr, nc, gh, gw, H = case
    x, want_sum, _ = _problem(case)
    acc = _run(lib, dev, x, case, 0, [0, B * nr])
    acc = _run(lib, dev, x, case, 0, [0, nr, B * nr], acc=acc)
    X = x.reshape(B, nr, nc, H)
    want = want_sum.copy()
    for b in range(B):
        for i, (r0, r1) in enumerate(E.pool_regions(nr, gh)):
            for j, (c0, c1) in enumerate(E.pool_regions(nc, gw)):
                for h in range(H):
                    a = float(want_sum[b, i, j, h])
                    for r in range(r0, r1):
                        t = 0.0
                        for c in range(c0, c1):
                            t = t + float(X[b, r, c, h])
                        a = a + t
                    want[b, i, j, h] = a
    E.same_bits(acc.cpu().numpy(), want, "second pass onto the first")
