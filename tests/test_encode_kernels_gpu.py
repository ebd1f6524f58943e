"""The two C entries of encode() (include/prosper_hip.h: pm_encode_f64, pm_encode_exact_mca_f64) on the device,
from random log-joints and not from a model: pm_encode_f64 against tests/encode_reference.py and against pm_recon_expect_f64
on the same buffers, one smallest shape per branch of encode_kernel; pm_encode_exact_mca_f64 against NumPy enumeration.

Tolerances.  mean against pm_recon_expect_f64's out[:, :H]: bit for bit.  prob against NumPy: 1e-11 relative to the largest
entry, the bound tests/test_reconstruct_gpu.py holds the same read-out to (both sides f64, they differ by summation order
only).  pm_encode_exact_mca_f64: the row-relative 1e-11 of tests/test_reconstruct_exact_gpu.py."""
import ctypes

import numpy as np
import pytest
from scipy.special import logsumexp

import encode_reference as E
import recon_reference as R

pytestmark = pytest.mark.gpu

RTOL = 1e-11
SENTINEL = -77.25


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype == np.float64, what
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), what


def _padded(dev, arr, ld):
    """``arr`` (N, K) as the leading columns of an (N, ld) device tensor filled with a sentinel."""
    import torch
    t = torch.full((arr.shape[0], ld), SENTINEL, dtype=torch.float64, device=dev)
    t[:, :arr.shape[1]] = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float64)).to(dev)
    return t


def run(dev, X, H, blocks=(1.0,), soff=1, moff=None, cand=None, table=None, a=1.0, off=None, lse=None, pad=(0, 0, 0),
        det=False, expect=True):
    """pm_encode_f64 (and pm_recon_expect_f64 on the same device buffers): (mean, prob, expect's out[:, :H] or None)."""
    import torch
    from prosper_amd import _lib
    N, K = X.shape
    S = 0 if table is None else table.shape[0]
    Hp = 0 if table is None else table.shape[1]
    moff = soff + len(blocks) * H if moff is None else moff
    Xd = _padded(dev, X, K + pad[0])
    mean = torch.full((N, H + pad[1]), SENTINEL, dtype=torch.float64, device=dev)
    prob = torch.full((N, H + pad[2]), SENTINEL, dtype=torch.float64, device=dev)
    out = torch.full((N, H + pad[1]), SENTINEL, dtype=torch.float64, device=dev)
    dd = lambda v: None if v is None else torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(dev)
    off_d, lse_d, tab_d = dd(off), dd(lse), dd(table)
    cand_d = None if cand is None else torch.from_numpy(np.ascontiguousarray(cand, dtype=np.int32)).to(dev)
    bv = (ctypes.c_double * 8)(*([float(v) for v in blocks] + [0.0] * (8 - len(blocks))))
    head = (_ptr(Xd), K + pad[0], _ptr(lse_d), ctypes.c_double(a), _ptr(off_d), _ptr(cand_d), _ptr(tab_d), bv, N, H, Hp, K,
            soff, len(blocks), moff, S)
    _lib.call("pm_encode_f64", *head, _ptr(mean), H + pad[1], _ptr(prob), H + pad[2], _stream(), det=det)
    if expect:
        _lib.call("pm_recon_expect_f64", *head, _ptr(out), H + pad[1], H, -1, _stream(), det=det)
    torch.cuda.synchronize()
    mean, prob, out = mean.cpu().numpy(), prob.cpu().numpy(), out.cpu().numpy()
    for t in (mean, prob):                  # nothing is written past column H
        assert (t[:, H:] == SENTINEL).all()
    return mean[:, :H], prob[:, :H], out[:, :H] if expect else None


def _states(rng, S, Hp, values):
    """S distinct rows over ``values`` with at least one non-zero entry (fewer when the space is smaller)."""
    values = np.asarray(values, dtype=np.float64)
    seen, rows = set(), []
    for _ in range(100 * S):
        r = tuple(values[rng.randint(len(values), size=Hp)])
        if any(r) and r not in seen:
            seen.add(r)
            rows.append(r)
        if len(rows) == S:
            break
    return np.array(rows)


def _cands(rng, N, H, Hp):
    return np.stack([rng.choice(H, size=Hp, replace=False) for _ in range(N)]).astype(np.int32)


# (tag, N, H, H', S, block values, table values): every branch of encode_kernel at its smallest shape
#   H = 5 / 64 / 65 / 130      the lane-strided latent loop: one partial trip, one full trip, a second trip of one lane, a third
#   S = 10 / 70                 the state loop: one trip of ten lanes, a second trip of six
#   H' = 1 / 16                 the unrolled position loops at both ends (PM_MAX_HPRIME = 16)
#   nblocks = 0 / 1 / 2 / 7     TSC (no one-cause prefix), the binary models, DSC with values -1, +1 and with eight values
LAYOUTS = [("binary H=5 S=10", 37, 5, 4, 10, (1.0,), (0., 1.)),
           ("binary H=64 H'=16 S=70", 37, 64, 16, 70, (1.0,), (0., 1.)),
           ("ternary H=65 H'=1", 37, 65, 1, 10, (), (-1., 0., 1.)),
           ("two blocks H=130 S=70", 37, 130, 5, 70, (-1.0, 1.0), (-1., 0., 1.)),
           ("seven blocks H=5", 37, 5, 3, 10, (-3., -2., -1., 1., 2., 3., 4.), (-3., -2., -1., 0., 1., 2., 3., 4.)),
           ("binary N=1", 1, 5, 4, 10, (1.0,), (0., 1.))]


def _layout(tag, N, H, Hp, S, blocks, values, seed=0):
    rng = np.random.RandomState(seed + H + S)
    table = _states(rng, S, Hp, values)
    soff = 1 if blocks else 0
    K = soff + len(blocks) * H + table.shape[0]
    return 3.0 * rng.normal(size=(N, K)), _cands(rng, N, H, Hp), table, soff


@pytest.mark.parametrize("tag,N,H,Hp,S,blocks,values", LAYOUTS, ids=[c[0] for c in LAYOUTS])
@pytest.mark.parametrize("lse_given", [False, True], ids=["lse formed", "lse given"])
@pytest.mark.parametrize("pad", [(0, 0, 0), (3, 2, 5)], ids=["tight", "ld>K ldm>H ldp>H"])
def test_encode_against_numpy_and_recon_expect(dev, tag, N, H, Hp, S, blocks, values, lse_given, pad):
    X, cand, table, soff = _layout(tag, N, H, Hp, S, blocks, values)
    lse = logsumexp(X, axis=1) if lse_given else None
    mean, prob, out = run(dev, X, H, blocks, soff, None, cand, table, lse=lse, pad=pad)
    _bits(mean, out, tag)
    want_mean, want_prob = E.codes_from_lpj(X, 1.0, cand, H, blocks, soff, soff + len(blocks) * H, table)
    err = E.rel_err(prob, want_prob)
    print("pm_encode_f64 %-28s prob %.3e mean %.3e (bound %.1e)" % (tag, err, E.rel_err(mean, want_mean), RTOL))
    assert err <= RTOL and E.rel_err(mean, want_mean) <= RTOL
    assert prob.max() <= 1.0 and prob.min() >= 0.0
    if blocks == (1.0,) and set(values) == {0., 1.}:
        _bits(prob, mean, tag + ": binary layout")
    # the same bits from the deterministic library
    mean_d, prob_d, _ = run(dev, X, H, blocks, soff, None, cand, table, lse=lse, pad=pad, det=True, expect=False)
    _bits(mean_d, mean, tag + ": deterministic library")
    _bits(prob_d, prob, tag + ": deterministic library")


@pytest.mark.parametrize("H", [5, 65])
def test_row_softmax_the_mixtures_mode(dev, H):
    """S = 0, H' = 0, one block of value 1 from column 0, a != 1 and column offsets: both outputs are softmax(a X + o)."""
    rng = np.random.RandomState(H)
    N = 37
    X, off = 5.0 * rng.uniform(size=(N, H)), rng.normal(size=H)
    mean, prob, out = run(dev, X, H, (1.0,), 0, None, None, None, a=-0.5, off=off, pad=(1, 0, 3))
    _bits(mean, out)
    _bits(prob, mean)
    want = R.softmax_rows(-0.5 * X + off[None, :])
    assert E.rel_err(prob, want) <= RTOL


def test_repeated_candidates_union_in_prob_both_positions_in_mean(dev):
    rng = np.random.RandomState(5)
    N, H, Hp = 50, 6, 4
    table = _states(rng, 70, Hp, (-1., 0., 1.))
    cand = _cands(rng, N, H, Hp)
    cand[:, 2] = cand[:, 0]                              # every row holds one latent at positions 0 and 2 ...
    cand[::7, 3] = cand[::7, 0]                          # ... and every seventh at 3 as well
    X = 3.0 * rng.normal(size=(N, table.shape[0]))
    heavy = int(np.nonzero((table[:, 0] != 0) & (table[:, 2] != 0))[0][0])
    X[::2, heavy] += 12.0                                # half the rows: a state non-zero at both positions dominates
    mean, prob, out = run(dev, X, H, (), 0, 0, cand, table)
    _bits(mean, out)
    want_mean, want_prob = E.codes_from_lpj(X, 1.0, cand, H, (), 0, 0, table)
    _, naive = E.codes_from_lpj(X, 1.0, cand, H, (), 0, 0, table, naive=True)
    assert naive.max() > 1.5                             # summing the positions would exceed 1: the rows test the rule
    assert E.rel_err(prob, want_prob) <= RTOL and E.rel_err(mean, want_mean) <= RTOL
    assert prob.max() <= 1.0 and prob.min() >= 0.0


def test_column_of_minus_infinity_and_nan_row(dev):
    tag, N, H, Hp, S, blocks, values = LAYOUTS[0]
    X, cand, table, soff = _layout(tag, N, H, Hp, S, blocks, values)
    X[:, 2] = -np.inf                                    # a one-cause column ...
    X[:, 1 + H + 3] = -np.inf                            # ... and a table state of zero weight
    mean, prob, out = run(dev, X, H, blocks, soff, None, cand, table)
    assert np.isfinite(mean).all() and np.isfinite(prob).all()
    _bits(mean, out)
    want_mean, want_prob = E.codes_from_lpj(X, 1.0, cand, H, blocks, soff, 1 + H, table)
    assert E.rel_err(prob, want_prob) <= RTOL and E.rel_err(mean, want_mean) <= RTOL
    Xn = X.copy()
    Xn[7, 1 + H + 5] = np.nan
    mean_n, prob_n, _ = run(dev, Xn, H, blocks, soff, None, cand, table, expect=False)
    assert np.isnan(mean_n[7]).all() and np.isnan(prob_n[7]).all()
    keep = np.arange(N) != 7
    _bits(mean_n[keep], mean[keep])
    _bits(prob_n[keep], prob[keep])
    # without one-cause blocks (TSC) a latent outside the row's candidates takes no value from any column: NaN all the same
    tag, N, H, Hp, S, blocks, values = LAYOUTS[2]
    X, cand, table, soff = _layout(tag, N, H, Hp, S, blocks, values)
    X[7, 0] = np.nan
    mean_n, prob_n, _ = run(dev, X, H, blocks, soff, None, cand, table, expect=False)
    assert np.isnan(mean_n[7]).all() and np.isnan(prob_n[7]).all()
    assert np.isfinite(mean_n[keep]).all() and np.isfinite(prob_n[keep]).all()


def test_second_trip_of_the_row_loop(dev):
    """N = 4 * 8192 + 5 at H = 4: the first five wavefronts take a second row.  The tail rows against NumPy, and every row
    bit for bit against the same rows sent as separate calls of 4096."""
    tag, N, H, Hp, S, blocks, values = "second trip", 4 * 8192 + 5, 4, 3, 4, (1.0,), (0., 1.)
    X, cand, table, soff = _layout(tag, N, H, Hp, S, blocks, values)
    mean, prob, out = run(dev, X, H, blocks, soff, None, cand, table)
    _bits(mean, out)
    tail = slice(4 * 8192 - 40, N)
    want_mean, want_prob = E.codes_from_lpj(X[tail], 1.0, cand[tail], H, blocks, soff, 1 + H, table)
    assert E.rel_err(prob[tail], want_prob) <= RTOL and E.rel_err(mean[tail], want_mean) <= RTOL
    for i in range(0, N, 4096):
        m, p, _ = run(dev, X[i:i + 4096], H, blocks, soff, None, cand[i:i + 4096], table, expect=False)
        _bits(m, mean[i:i + 4096])
        _bits(p, prob[i:i + 4096])


# -------------------------------------------------------------------------------------------- pm_encode_exact_mca_f64
def run_exact_mca(dev, Y, W, rho, signed, pi, sigma, det=False, lde=None):
    import torch
    from prosper_amd import _lib
    N, D = Y.shape
    H = W.shape[1]
    Wt = np.ascontiguousarray(W.T)
    Wrho = np.sign(Wt) * np.abs(Wt) ** rho if signed else Wt ** rho
    lde = H if lde is None else lde
    lib = _lib.load(det)
    work = torch.empty(int(lib.pm_recon_exact_work_len(N, H, D)), dtype=torch.float64, device=dev)
    Yd = torch.from_numpy(np.ascontiguousarray(Y)).to(dev)
    Wd = torch.from_numpy(np.ascontiguousarray(Wrho)).to(dev)
    out = torch.full((N, lde), SENTINEL, dtype=torch.float64, device=dev)
    dbl = ctypes.c_double
    _lib.call("pm_encode_exact_mca_f64", _ptr(Yd), D, _ptr(Wd), dbl(1. / rho), int(signed), dbl(np.log(pi)),
              dbl(np.log(1 - pi)), dbl(1. / sigma ** 2), N, D, H, _ptr(out), lde, _ptr(work), _stream(), det=det)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert (out[:, H:] == SENTINEL).all()
    return out[:, :H]


# (H, D, N): H = 1 (two states), 6 (64 states: one range), 7 (two ranges), 13 (64 ranges); D = 1, one full slab of 64
# dimensions, 65 (a second slab of one lane), 130 (three); N = 1, one full row block of 64, 65 (a second block of one row)
EXACT = [(1, 1, 1), (6, 64, 64), (7, 65, 65), (13, 130, 5)]


@pytest.mark.parametrize("H,D,N", EXACT)
@pytest.mark.parametrize("signed", [False, True], ids=["mca", "mmca"])
def test_encode_exact_mca_against_enumeration(dev, H, D, N, signed):
    rng = np.random.RandomState(31 * H + D)
    W = rng.uniform(-2, 3, size=(D, H)) if signed else rng.uniform(0.1, 3, size=(D, H))
    W = np.where(np.abs(W) < 0.05, 0.05, W)
    pi, sigma, rho = 0.25, 0.7, (6.0 if signed else 21.0)
    mean_fn = R.mca_mean(W, rho, signed)
    Y = np.array([mean_fn(np.nonzero(s)[0]) for s in rng.uniform(size=(N, H)) < pi]) + sigma * rng.normal(size=(N, D))
    got = run_exact_mca(dev, Y, W, rho, signed, pi, sigma, lde=H + 3)
    want, want_prob = E.enum_mca(Y, W, rho, signed, pi, sigma)
    err = R.row_rel_err(got, want)
    print("pm_encode_exact_mca_f64 %s H=%d D=%d N=%d: row-relative error %.3e (bound %.1e)"
          % ("mmca" if signed else "mca", H, D, N, err, RTOL))
    assert err <= RTOL
    _bits(want, want_prob)                               # (binary latents: the reference's two marginals coincide)
    _bits(run_exact_mca(dev, Y, W, rho, signed, pi, sigma, det=True), got, "deterministic library")
    n = N // 2
    _bits(run_exact_mca(dev, Y[n:n + 1], W, rho, signed, pi, sigma), got[n:n + 1], "a row sent alone")
