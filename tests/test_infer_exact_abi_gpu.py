"""The exact top-K kernels (infer_exact.hip, pm_exact.h) through the C ABI -- pm_infer_exact_lin_f64, pm_infer_exact_mca_f64 --
from both libraries, one case per cell of pm_infer_exact_plan (tests/test_infer_exact_cpu.py pins the case tables to the plan
and fails for a cell without a case), against the longdouble reference tests/infer_exact_reference.py on the kernels' own
operands (tests/exact_kernels_reference.py: values that are no integers, a prior row per latent, one -inf prior entry).

Harness.  Y has a row stride above D and NaN in its padding.  top_idx, top_l and v are larger than needed and filled with a
sentinel that must survive past `cols` and past N; `work` is work_len + 64 doubles whose last 64 must survive.  Every random
case runs four times -- default library; again; deterministic library under other strides; rows permuted -- and must return the
same bits per row.  State indices are compared for equality, top_l and v to 1e-11 of the row's largest compared magnitude
(floor 1): RTOL of tests/test_exact_kernels_gpu.py.  The reference asserts, for every row of every random case, that
consecutive entries among the topK + 1 best differ by more than 1e-9 max(1, |l|) in its own values, so rounding cannot swap
neighbours; no row is left out of a comparison.  The planted cases need no margin: their log-joints are small integers, exact
in every arithmetic, and the expected order is pure tie-breaking by index.
"""
import ctypes

import numpy as np
import pytest

import exact_kernels_reference as R
import infer_exact_reference as IR

pytestmark = pytest.mark.gpu

RTOL = 1e-11
SENT = -12345.678
ISENT = -777
LIN, MCA = R.LIN, R.MCA


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _lib_of(det):
    from prosper_amd import _lib
    return _lib.load(det)


def _up(a, dev):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _run(kind, det, op, Y, topK, dev, pad=3):
    """One call of the kind's entry: (idx (N, cols), l (N, cols), v (N,)) as NumPy, after the sentinel checks."""
    import torch
    from prosper_amd import _lib
    lib = _lib_of(det)
    N, D = Y.shape
    H = op["logp"].shape[0] if kind == LIN else op["Wrho"].shape[0]
    K = op["K"] if kind == LIN else 0
    plan = (ctypes.c_int64 * IR.PLAN_LEN)()
    assert lib.pm_infer_exact_plan(kind, N, D, K, H, topK, plan) == 0
    assert list(plan) == IR.infer_plan(kind, N, D, K, H, topK)[1]
    cols = plan[6]
    ldy, ld = D + pad, topK + pad
    Yb = torch.full((max(N, 1), ldy), float("nan"), dtype=torch.float64, device=dev)
    Yb[:N, :D] = _up(Y, dev)
    idx = torch.full((N + 1, ld), ISENT, dtype=torch.int64, device=dev)
    tl = torch.full((N + 1, ld), SENT, dtype=torch.float64, device=dev)
    v = torch.full((N + 2,), SENT, dtype=torch.float64, device=dev)
    wl = int(lib.pm_infer_exact_work_len(N, H, topK))
    work = torch.full((wl + 64,), SENT, dtype=torch.float64, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = (topK, _ptr(idx), ld, _ptr(tl), ld, _ptr(v), _ptr(work), st)
    if kind == LIN:
        t = {k: _up(op[k], dev) for k in ("ymu", "P", "G", "logp", "values")}
        _lib.call("pm_infer_exact_lin_f64", _ptr(Yb), ldy, _ptr(t["ymu"]), _ptr(t["P"]), _ptr(t["G"]), _ptr(t["logp"]),
                  _ptr(t["values"]), K, N, D, H, *out, det=det)
    else:
        Wr = _up(op["Wrho"], dev)
        _lib.call("pm_infer_exact_mca_f64", _ptr(Yb), ldy, _ptr(Wr), ctypes.c_double(op["inv_rho"]), int(op["signed"]),
                  ctypes.c_double(op["lp1"]), ctypes.c_double(op["lp0"]), ctypes.c_double(op["inv_s2"]), N, D, H, *out, det=det)
    torch.cuda.synchronize()
    idx, tl, v, work = idx.cpu().numpy(), tl.cpu().numpy(), v.cpu().numpy(), work.cpu().numpy()
    assert np.all(idx[:, cols:] == ISENT) and np.all(idx[N:] == ISENT), "index columns past cols / rows past N were written"
    assert np.all(tl[:, cols:] == SENT) and np.all(tl[N:] == SENT) and np.all(v[N:] == SENT)
    assert np.all(work[wl:] == SENT), "the workspace was overrun"
    return idx[:N, :cols], tl[:N, :cols], v[:N]


def _same(a, b):
    return all(np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y)
               for x, y in zip(a, b))


def _compare(got, want, what):
    idx, tl, v = got
    ridx, rl, rv = want
    assert np.array_equal(idx, ridx), "%s: state indices differ in rows %s" % (what, np.nonzero((idx != ridx).any(axis=1))[0])
    rl64, rv64 = np.asarray(rl, dtype=np.float64), np.asarray(rv, dtype=np.float64)
    fin = np.isfinite(rl64)
    assert np.array_equal(tl[~fin], rl64[~fin]), what                      # -inf where the reference has -inf
    scale = np.maximum(1.0, np.max(np.where(fin, np.abs(rl64), 0.0), axis=1, initial=0.0))
    err = np.max(np.where(fin, np.abs(np.where(fin, tl, 0.0) - np.where(fin, rl64, 0.0)), 0.0) / scale[:, None], initial=0.0)
    errv = np.max(np.abs(v - rv64) / np.maximum(1.0, np.abs(rv64)), initial=0.0)
    print("%s: top_l %.3e  v %.3e (bound %.0e)" % (what, err, errv, RTOL))
    assert err <= RTOL and errv <= RTOL, (what, err, errv)


def _four_runs(kind, op, Y, topK, dev, want, what):
    first = _run(kind, False, op, Y, topK, dev)
    _compare(first, want, what)
    assert _same(first, _run(kind, False, op, Y, topK, dev)), what + ": a second call differs"
    assert _same(first, _run(kind, True, op, Y, topK, dev, pad=5)), what + ": the deterministic library differs"
    perm = np.random.RandomState(9).permutation(Y.shape[0])
    assert _same([x[perm] for x in first], _run(kind, False, op, Y[perm], topK, dev)), what + ": a row permutation differs"


@pytest.mark.parametrize("case", IR.LIN_CASES, ids=lambda c: "K%d_H%d_N%d_top%d" % c[:4])
def test_lin_cases(case, dev):
    K, H, N, topK, seed = case
    op = R.lin_operands(np.random.RandomState(seed), 5, H, K, N)
    want = IR.lin_top(op["Y"], op["ymu"], op["P"], op["G"], op["logp"], op["values"], topK)        # (asserts the margin)
    _four_runs(LIN, op, op["Y"], topK, dev, want, "lin %r" % (case,))


@pytest.mark.parametrize("case", IR.MCA_CASES, ids=lambda c: "%s_H%d_N%d_D%d_top%d" % ((("mca", "mmca")[c[0]],) + c[1:5]))
def test_mca_cases(case, dev):
    signed, H, N, D, topK, seed = case
    op = R.mca_operands(np.random.RandomState(seed), D, H, N, signed)
    want = IR.mca_top(op["Y"], op["Wrho"], op["inv_rho"], op["signed"], op["lp1"], op["lp0"], op["inv_s2"], topK)
    _four_runs(MCA, op, op["Y"], topK, dev, want, "mca %r" % (case,))


# Planted winners.  K = 2, H = 14: L = 10, CH = 1024, 16 chunks in 8 ranges of 2048 states.  t sits at the first and last
# state and either side of a lane (0 | 1), wavefront (63 | 64), thread-block (255 | 256: a thread's next lo state), chunk
# (1023 | 1024) and range (2047 | 2048) boundary.  K = 3, H = 8: CH = 729 (a ragged last lo slot), 9 chunks in 4 ranges.
PLANTED = [(2, 14, t) for t in (0, 1, 63, 64, 255, 256, 1023, 1024, 2047, 2048, 2 ** 14 - 1)] + \
          [(3, 8, t) for t in (728, 729, 2 * 729 - 1, 2 * 729, 3 ** 8 - 1)]


@pytest.mark.parametrize("K,H,t", PLANTED)
def test_planted_winner_is_pure_tie_breaking(K, H, t, dev):
    ops, dist = IR.planted_lin(K, H, t)
    topK = IR.MAX_TOPK
    Y = np.tile(ops["ymu"], (2, 1))
    widx, wscore = IR.planted_order(dist, topK)
    for det in (False, True):
        idx, tl, v = _run(LIN, det, ops, Y, topK, dev)
        for n in range(2):
            assert np.array_equal(idx[n], widx), (det, n, idx[n], widx)
            assert np.array_equal(tl[n], -wscore.astype(np.float64))
        rv = np.asarray(R.lse_rows(-dist[None, :].astype(IR.LD))[0], dtype=np.float64)
        assert np.all(np.abs(v - rv) <= RTOL * np.maximum(1.0, np.abs(rv)))


@pytest.mark.parametrize("H,signed", [(6, 0), (11, 1), (7, 0)])
def test_planted_mca_orders_by_population_count(H, signed, dev):
    """inv_s2 = 0, lp1 = -1, lp0 = 0: l = -|s| exactly, so the order is (population count, index)."""
    op = R.mca_operands(np.random.RandomState(0), 7, H, 3, signed)
    op.update(lp1=-1.0, lp0=0.0, inv_s2=0.0)
    pc = IR.popcounts(H)
    widx, wscore = IR.planted_order(pc, IR.MAX_TOPK)
    for det in (False, True):
        idx, tl, v = _run(MCA, det, op, op["Y"], IR.MAX_TOPK, dev)
        for n in range(3):
            assert np.array_equal(idx[n], widx) and np.array_equal(tl[n], -wscore.astype(np.float64))


def test_zero_prior_states_come_last_by_index(dev):
    rng = np.random.RandomState(4)
    op = R.lin_operands(rng, 5, 3, 2, 4, neg_inf=False)
    op["logp"][1, 1] = -np.inf                                # the states with bit 1 set: 2, 3, 6, 7
    want = IR.lin_top(op["Y"], op["ymu"], op["P"], op["G"], op["logp"], op["values"], 8)
    got = _run(LIN, False, op, op["Y"], 8, dev)
    _compare(got, want, "lin zero prior")
    for n in range(4):
        assert sorted(got[0][n, :4]) == [0, 1, 4, 5] and list(got[0][n, 4:]) == [2, 3, 6, 7]
        assert np.all(np.isfinite(got[1][n, :4])) and np.all(got[1][n, 4:] == -np.inf)
    # with a shorter list the -inf states stay out
    assert np.array_equal(_run(LIN, False, op, op["Y"], 4, dev)[0], got[0][:, :4])
    for lp1, lp0, finite in ((-np.inf, np.log(0.7), 0), (np.log(0.3), -np.inf, 7)):
        mop = R.mca_operands(rng, 6, 3, 3, 0, lp1=lp1, lp0=lp0)
        want = IR.mca_top(mop["Y"], mop["Wrho"], mop["inv_rho"], 0, lp1, lp0, mop["inv_s2"], 8)
        got = _run(MCA, False, mop, mop["Y"], 8, dev)
        _compare(got, want, "mca zero prior")
        rest = [i for i in range(8) if i != finite]
        for n in range(3):
            assert list(got[0][n]) == [finite] + rest and np.all(got[1][n, 1:] == -np.inf)


@pytest.mark.parametrize("kind", [LIN, MCA], ids=["lin", "mca"])
def test_a_nan_row_is_flagged_and_no_other_row_changes(kind, dev):
    rng = np.random.RandomState(5)
    if kind == LIN:
        op = R.lin_operands(rng, 5, 12, 2, 6)
    else:
        op = R.mca_operands(rng, 5, 7, 6, 0)
    clean = _run(kind, False, op, op["Y"], 10, dev)
    Y = op["Y"].copy()
    Y[2, 3] = np.nan
    for det in (False, True):
        idx, tl, v = _run(kind, det, op, Y, 10, dev)
        assert np.all(idx[2] == -1) and np.all(np.isnan(tl[2])) and np.isnan(v[2])
        keep = [0, 1, 3, 4, 5]
        assert _same([x[keep] for x in clean], [idx[keep], tl[keep], v[keep]])
