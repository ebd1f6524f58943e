"""tests/exact_kernels_reference.py pinned without a device, and the host side of the exact-enumeration entries
(pm_loglik_exact_plan, pm_recon_exact_plan: the functions the six launchers take their launch from) swept over every shape.

The reference is pinned three ways: on the brute-force functions of tests/test_loglik_exact_gpu.py and
tests/recon_reference.py at operands built from model parameters (float64 NumPy, dense slogdet / solve for GSC: 1e-11); on
its own factorised closed forms at small H, where enumeration and closed form are both available (longdouble: 2e-15); and
total_fixed_order on exactly representable rows.

Plan sweep, both library builds: N in 0..600 and {1023, 1024, 1025, 200000}, every (K, H) with K^H <= 2^32 and H <= 32, every
H <= 32 for MCA and H <= 16 for GSC (recon MCA also over D in {1, 64, 65, 1024}).  The C plan equals the Python restatement
written from the header; the ranges [space r / R, space (r + 1) / R) partition the index space; 1 <= R <= units; the partials'
offset plus length stays inside pm_loglik_exact_work_len / pm_recon_exact_work_len -- the memory-safety invariant of the work
buffers --; CH <= 1024 and 3 L <= 32 (a packed code fits 32 bits).

Cells no valid input reaches (asserted in test_no_range_is_empty): a range with c0 == c1 needs more ranges than units, and R
is capped by the units in both files, so no launch of either unit has an empty range; in recon_exact.hip R equals the size
of the space only where the space is one chunk (the linear kernels at H <= L)."""
import ctypes

import numpy as np
import pytest

import exact_kernels_reference as R
import recon_reference as RR
import test_loglik_exact_gpu as TL

LD = np.longdouble
KINDS = (R.LIN, R.MCA, R.GSC)
SWEEP_N = list(range(0, 601)) + [1023, 1024, 1025, 200000]
LIN_SHAPES = [(K, H) for K in range(2, 9) for H in range(1, 33) if K ** H <= 2 ** 32]
FAKE = ctypes.c_void_p(0x1000)       # never dereferenced: every entry call below fails its argument check


@pytest.fixture(scope="module", params=[False, True], ids=["default", "deterministic"])
def lib(request):
    from prosper_amd import _lib
    return _lib.load(det=request.param)


def _plan(lib, unit, kind, N, D, K, H):
    out = (ctypes.c_int64 * R.PLAN_LEN)(*([-7] * R.PLAN_LEN))
    rc = getattr(lib, "pm_%s_exact_plan" % unit)(kind, N, D, K, H, out)
    return rc, list(out)


def _rel(got, want):
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), LD(1e-300))))


# ------------------------------------------------------------------------------------- the reference on model parameters
def test_entries_exported(lib):
    from prosper_amd import _lib
    assert lib.pm_version() >= 1031 and _lib.MIN_VERSION >= 1031
    for name in ("pm_loglik_exact_plan", "pm_recon_exact_plan"):
        assert name in _lib.SIGNATURES
        getattr(lib, name)


@pytest.mark.parametrize("K,H", [(2, 7), (3, 5), (4, 4)])
def test_linear_reference_on_model_parameters(K, H):
    rng = np.random.RandomState(10 * K + H)
    D, N = 6, 9
    W, sigma, mu = rng.normal(size=(D, H)), 0.9, rng.normal(size=D) * 0.2
    values = {2: [0., 1.], 3: [-1., 0., 1.], 4: [0., 1., 2., 3.]}[K]
    pi = rng.dirichlet(np.ones(K) * 3)
    Y = rng.normal(size=(N, D)) * 1.5
    ops = (W / sigma ** 2, W.T @ W / sigma ** 2, np.tile(np.log(pi), (H, 1)), values)
    rows = R.lin_rows(Y, mu, *ops, -0.5 * D * np.log(2 * np.pi * sigma ** 2), -0.5 / sigma ** 2)
    assert _rel(rows, TL._brute_linear(Y - mu, W, sigma, values, np.log(pi))) < 1e-11
    yhat = mu[None, :] + R.lin_means(Y, mu, *ops) @ W.T
    assert RR.row_rel_err(np.asarray(yhat, dtype=np.float64), RR.enum_linear(Y, W, sigma, values, np.log(pi), mu=mu)) < 1e-11


@pytest.mark.parametrize("signed", [False, True])
def test_mca_reference_on_model_parameters(signed):
    rng = np.random.RandomState(31 + signed)
    D, H, N, pi, sigma = 7, 6, 8, 0.25, 0.7
    rho = 6.0 if signed else 21.0
    W = rng.uniform(-2, 3, size=(D, H)) if signed else rng.uniform(0.1, 3, size=(D, H))
    Y = rng.normal(size=(N, D)) + 1.0
    Wrho = (np.sign(W) * np.abs(W) ** rho).T
    ops = (Wrho, 1.0 / rho, int(signed), np.log(pi), np.log(1 - pi), 1.0 / sigma ** 2)
    rows = R.mca_rows(Y, *ops, -0.5 * D * np.log(2 * np.pi * sigma ** 2))
    assert _rel(rows, TL._brute_binary(Y, H, TL._bsc_prior(H, pi), TL._mca_mean(W, rho, signed), sigma ** 2)) < 1e-11
    assert RR.row_rel_err(np.asarray(R.mca_means(Y, *ops), dtype=np.float64), RR.enum_mca(Y, W, rho, signed, pi, sigma)) < 1e-11


@pytest.mark.parametrize("kind", ["scalar", "diagonal", "full"])
def test_gsc_reference_on_the_dense_formula(kind):
    """... slogdet and solve of C_s = Sigma + W_s Psi_s W_s^T per support (TL._gsc_brute, RR.enum_gsc)."""
    rng = np.random.RandomState(40 + len(kind))
    D, H, N = 6, 5, 7
    p = TL._gsc_params(rng, D, H, kind)
    Y = rng.normal(size=(N, D)) * 1.5
    Sig = RR._gsc_sigma(p, D)
    Si = np.linalg.inv(Sig)
    P, M = Si @ p["W"], p["W"].T @ Si @ p["W"]
    wdiag = None if kind == "full" else np.diag(Si).copy()
    Lw = np.linalg.inv(np.linalg.cholesky(Sig)) if kind == "full" else None
    logp = np.stack([np.log(1 - p["pi"]), np.log(p["pi"])], axis=1)
    cst = -0.5 * D * np.log(2 * np.pi) - 0.5 * np.linalg.slogdet(Sig)[1]
    rows = R.gsc_rows(Y, P, wdiag, Lw, M, p["psi_sq"], p["mu"], logp, cst)
    assert _rel(rows, TL._gsc_brute(p, Y)) < 1e-11
    yhat = R.gsc_means(Y, P, M, p["psi_sq"], p["mu"], logp) @ p["W"].T
    assert RR.row_rel_err(np.asarray(yhat, dtype=np.float64), RR.enum_gsc(p, Y)) < 1e-11


# ----------------------------------------------------------------------------- closed forms against enumeration, small H
def test_linear_closed_form_equals_enumeration():
    rng = np.random.RandomState(50)
    blocks = [[0, 4], [2, 3, 1], [5]]
    o = R.lin_operands(rng, 5, 6, 3, 6, blocks=blocks)
    a = (o["Y"], o["ymu"], o["P"], o["G"], o["logp"], o["values"])
    assert np.count_nonzero(o["G"]) == 4 + 9 + 1 and np.isinf(o["logp"]).sum() == 1
    assert _rel(R.lin_block_rows(*a, o["cst"], o["qcoef"], blocks), R.lin_rows(*a, o["cst"], o["qcoef"])) < 2e-15
    assert RR.row_rel_err(R.lin_block_means(*a, blocks), R.lin_means(*a)) < 2e-15


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("edge", ["none", "lp1", "lp0"])
def test_mca_closed_form_equals_enumeration(signed, edge):
    rng = np.random.RandomState(51)
    o = R.mca_operands(rng, 9, 5, 6, signed, disjoint=True, lp1=-np.inf if edge == "lp1" else np.log(0.3),
                       lp0=-np.inf if edge == "lp0" else np.log(0.7))
    a = (o["Y"], o["Wrho"], o["inv_rho"], o["signed"], o["lp1"], o["lp0"], o["inv_s2"])
    assert _rel(R.mca_disjoint_rows(*a, o["cst"]), R.mca_rows(*a, o["cst"])) < 2e-15
    assert RR.row_rel_err(R.mca_disjoint_means(*a), R.mca_means(*a)) < 2e-15


def test_gsc_closed_form_equals_enumeration():
    rng = np.random.RandomState(52)
    blocks = [[0, 3], [1, 2, 5], [4]]
    o = R.gsc_operands(rng, 5, 6, 6, noise="Lw", blocks=blocks)
    assert np.isinf(o["logp"]).sum() == 2
    assert _rel(R.gsc_block_rows(o["Y"], o["P"], o["wdiag"], o["Lw"], o["M"], o["Psi"], o["mu"], o["logp"], o["cst"], blocks),
                R.gsc_rows(o["Y"], o["P"], o["wdiag"], o["Lw"], o["M"], o["Psi"], o["mu"], o["logp"], o["cst"])) < 2e-15
    assert RR.row_rel_err(R.gsc_block_means(o["Y"], o["P"], o["M"], o["Psi"], o["mu"], o["logp"], blocks),
                          R.gsc_means(o["Y"], o["P"], o["M"], o["Psi"], o["mu"], o["logp"])) < 2e-15


def test_gsc_reference_indefinite_block_gives_nan_rows():
    o = R.gsc_operands(np.random.RandomState(53), 4, 3, 3, pi_edge=False)
    o["Psi"][0, 1] = o["Psi"][1, 0] = 3.0 * np.sqrt(o["Psi"][0, 0] * o["Psi"][1, 1])
    assert np.isnan(R.gsc_rows(o["Y"], o["P"], None, None, o["M"], o["Psi"], o["mu"], o["logp"], 0.0)).all()
    assert np.isnan(R.gsc_means(o["Y"], o["P"], o["M"], o["Psi"], o["mu"], o["logp"])).all()


def test_straddling_blocks():
    for (K, H), cell in list(R.LIN_DEPTH.items()) + list(R.LIN_BOUND.items()):
        L = cell[0]
        blocks = R.straddling_blocks(H, L)
        assert sorted(h for b in blocks for h in b) == list(range(H)) and [L - 1, L, H - 1] in blocks
        assert all(1 <= len(b) <= 3 for b in blocks)
        across = [len(b) for b in blocks if min(b) < L <= max(b)]                   # blocks across the lo / hi boundary
        assert len(across) >= 3 and {2, 3} <= set(across), (K, H, blocks)


def test_total_fixed_order():
    rows = np.arange(1, 601, dtype=np.float64) * 0.125                   # exact in any order
    assert R.total_fixed_order(rows) == rows.sum() and R.total_fixed_order(rows[:0]) == 0.0
    x = np.zeros(257)
    x[0], x[256], x[1] = 1.0, 2.0 ** -53, 2.0 ** -53                       # row 256 joins row 0 before the tree: lost there
    assert R.total_fixed_order(x) == 1.0 and R.total_fixed_order(x[[1, 0] + list(range(2, 257))]) == 1.0 + 2.0 ** -52


# ----------------------------------------------------------------------------------------------------------- plan sweep
def _shapes():
    for K, H in LIN_SHAPES:
        yield R.LIN, K, H, (5,)
    for H in range(1, 33):
        yield R.MCA, 0, H, (1, 64, 65, 1024)
    for H in range(1, 17):
        yield R.GSC, 0, H, (5,)


def test_plan_sweep(lib):
    seen = set()
    for kind, K, H, Ds in _shapes():
        for N in SWEEP_N:
            rc, p = _plan(lib, "loglik", kind, N, Ds[0], K, H)
            assert (rc, p) == R.loglik_plan(kind, N, Ds[0], K, H), (kind, N, K, H, p)
            tn, L, CH, space, units, Rr, grid, off, length = p[:9]
            assert 1 <= Rr <= units and CH <= 1024 and 3 * L <= 32 and grid == -(-N // tn) * Rr
            assert off + length <= lib.pm_loglik_exact_work_len(N, H), (kind, N, K, H, p)
            assert off >= N * (H + 2) and length == 2 * N * Rr
            seen.add((space, Rr))
        for D in Ds:
            for N in SWEEP_N if D == Ds[0] else (0, 1, 63, 64, 65, 200000):
                rc, p = _plan(lib, "recon", kind, N, D, K, H)
                assert (rc, p) == R.recon_plan(kind, N, D, K, H), (kind, N, D, K, H, p)
                rows, blocks, L, CH, space, Rr, slabs, off, len1, len2 = p
                assert 1 <= Rr <= space and CH <= 1024 and 3 * L <= 32 and blocks == -(-N // rows)
                assert off + max(len1, len2) <= lib.pm_recon_exact_work_len(N, H, D), (kind, N, D, K, H, p)
                assert slabs == (-(-D // 64) if kind == R.MCA else 0) and slabs <= 16
                seen.add((space, Rr))
    for space, Rr in seen:                            # the ranges partition the space, and none is empty
        edges = np.arange(Rr + 1, dtype=np.int64) * space // Rr
        assert edges[0] == 0 and edges[-1] == space and np.all(np.diff(edges) >= 1), (space, Rr)
        assert R.ranges(space, Rr)[0][0] == 0 and R.ranges(space, Rr)[-1][1] == space


def test_no_range_is_empty(lib):
    """The cell `c0 == c1` is unreachable: R <= units <= space in loglik_exact.hip and R <= space in recon_exact.hip, for every
    shape and N (an empty range needs space < R).  recon_exact.hip: R == space only at one chunk."""
    for kind, K, H, Ds in _shapes():
        for N in (0, 1, 2, 15, 16, 63, 64, 600, 200000):
            p = _plan(lib, "loglik", kind, N, Ds[0], K, H)[1]
            assert p[5] <= p[4] <= p[3]
            q = _plan(lib, "recon", kind, N, Ds[0], K, H)[1]
            assert q[5] <= q[4] and (q[5] < q[4] or q[4] == 1)
            assert (q[4] == 1) == (kind == R.LIN and H == q[2])


def test_case_table_cells(lib):
    """Every literal cell the GPU module names is what the plan reports."""
    for (K, H), (L, CH, chunks) in R.LIN_CELLS.items():
        for N in R.LIN_LOGLIK_N:
            p = _plan(lib, "loglik", R.LIN, N, 5, K, H)[1]
            assert p[:4] == [8 if N >= 64 else 1, L, CH, chunks], (K, H, N, p)
        for N in R.LIN_RECON_N:
            p = _plan(lib, "recon", R.LIN, N, 5, K, H)[1]
            assert p[:5] == [256, 2 if N == 257 else 1, L, CH, chunks], (K, H, N, p)
    for (K, H), (L, CH, chunks, r_ll, r_rx) in R.LIN_DEPTH.items():
        assert _plan(lib, "loglik", R.LIN, 2, 5, K, H)[1][:6] == [1, L, CH, chunks, chunks, r_ll]
        assert _plan(lib, "recon", R.LIN, 2, 5, K, H)[1][2:6] == [L, CH, chunks, r_rx]
    for (K, H), (L, CH, chunks, r_ll) in R.LIN_BOUND.items():
        assert _plan(lib, "loglik", R.LIN, 2, 5, K, H)[1][:6] == [1, L, CH, chunks, chunks, r_ll]
        assert _plan(lib, "loglik", R.LIN, 2, 5, K, H + 1)[0] == R.PM_ERANGE
    for N in R.MCA_LOGLIK_N:
        assert _plan(lib, "loglik", R.MCA, N, 7, 0, 6)[1][0] == (4 if N >= 16 else 1)
    for N in R.MCA_RECON_N:
        assert _plan(lib, "recon", R.MCA, N, 5, 0, 6)[1][:2] == [64, 2 if N == 65 else 1]
    for D in R.MCA_RECON_D + (1024,):
        assert _plan(lib, "recon", R.MCA, 3, D, 0, 6)[1][6] == {1: 1, 63: 1, 64: 1, 65: 2, 128: 2, 1024: 16}[D]
    assert _plan(lib, "recon", R.MCA, 3, 1025, 0, 6)[0] == R.PM_ERANGE
    assert _plan(lib, "loglik", R.MCA, 3, 1025, 0, 6)[0] == R.PM_OK
    for N in R.GSC_N + (257,):
        assert _plan(lib, "loglik", R.GSC, N, 5, 0, 5)[1][6] == -(-N // 64)                    # R = 1: the grid is the tiles
        assert _plan(lib, "recon", R.GSC, N, 5, 0, 5)[1][:2] == [256, 2 if N == 257 else 1]
    cells = {"R=1": set(), "R=cap": set(), "inside": set()}
    for (unit, kind, N, K, H), (Rr, cap) in R.RANGE_CELLS.items():
        p = _plan(lib, unit, kind, N, 20 if kind == R.MCA else 5, K, H)[1]
        assert (p[5], p[4]) == (Rr, cap), (unit, kind, N, K, H, p)
        cells["R=1" if Rr == 1 else "R=cap" if Rr == cap else "inside"].add((unit, kind))
    assert cells["R=1"] == cells["inside"] == {(u, k) for u in ("loglik", "recon") for k in KINDS}
    assert cells["R=cap"] == {("loglik", k) for k in KINDS}          # recon: only at one chunk, which is R = 1 (above)


# ------------------------------------------------------------------------------------------------------ argument codes
def test_plan_argument_codes(lib):
    out = (ctypes.c_int64 * R.PLAN_LEN)()
    for name in ("pm_loglik_exact_plan", "pm_recon_exact_plan"):
        f = getattr(lib, name)
        assert f(R.LIN, 4, 8, 2, 10, None) == R.PM_EINVAL
        for kind in KINDS:
            assert f(kind, 4, 8, 2, 10, out) == R.PM_OK and f(kind, 0, 1, 2, 1, out) == R.PM_OK
            assert f(kind, -1, 8, 2, 10, out) == R.PM_EINVAL
            assert f(kind, 4, 0, 2, 10, out) == R.PM_EINVAL
            assert f(kind, 4, 8, 2, 0, out) == R.PM_EINVAL
        for kind in (-1, 3):
            assert f(kind, 4, 8, 2, 10, out) == R.PM_EINVAL
        for K in (-1, 0, 1, 9):
            assert f(R.LIN, 4, 8, K, 10, out) == R.PM_EINVAL
            assert f(R.MCA, 4, 8, K, 10, out) == R.PM_OK and f(R.GSC, 4, 8, K, 10, out) == R.PM_OK       # K is not read
        for K, H in ((2, 33), (3, 21), (4, 17), (5, 14), (6, 13), (7, 12), (8, 11)):
            assert f(R.LIN, 4, 8, K, H, out) == R.PM_ERANGE and f(R.LIN, 4, 8, K, H - 1, out) == R.PM_OK
        assert f(R.LIN, 4, 8, 1, 40, out) == R.PM_EINVAL                  # a bad K before the bounds, as in the entries
        assert f(R.MCA, 4, 8, 0, 33, out) == R.PM_ERANGE and f(R.MCA, 4, 8, 0, 32, out) == R.PM_OK
        assert f(R.GSC, 4, 8, 0, 17, out) == R.PM_ERANGE and f(R.GSC, 4, 8, 0, 16, out) == R.PM_OK
    assert lib.pm_recon_exact_plan(R.MCA, 4, 1025, 0, 10, out) == R.PM_ERANGE
    assert lib.pm_recon_exact_plan(R.MCA, 4, 1024, 0, 10, out) == R.PM_OK
    assert lib.pm_recon_exact_plan(R.LIN, 4, 1025, 2, 10, out) == R.PM_OK


def test_plan_codes_are_the_entries_codes(lib):
    """For the same (N, D, K, H) the compute entries return what the plan returns (here: wherever that is a refusal, so that
    nothing reaches a device)."""
    out = (ctypes.c_int64 * R.PLAN_LEN)()
    for N, D, K, H in [(-1, 8, 2, 10), (4, 0, 2, 10), (4, 8, 2, 0), (4, 8, 9, 10), (4, 8, 1, 40), (4, 8, 2, 33), (4, 8, 3, 21),
                       (4, 8, 8, 11), (4, 8, 2, 17), (4, 1025, 2, 6)]:
        ldy = max(D, 1)
        entries = {
            ("loglik", R.LIN): lambda: lib.pm_loglik_exact_lin_f64(FAKE, ldy, None, FAKE, FAKE, FAKE, FAKE, K, 0.0, -0.5, N, D, H,
                                                                   None, FAKE, FAKE, None),
            ("loglik", R.MCA): lambda: lib.pm_loglik_exact_mca_f64(FAKE, ldy, FAKE, 0.1, 0, -1.0, -0.1, 1.0, 0.0, N, D, H, None,
                                                                   FAKE, FAKE, None),
            ("loglik", R.GSC): lambda: lib.pm_loglik_exact_gsc_f64(FAKE, ldy, FAKE, None, None, FAKE, FAKE, FAKE, FAKE, 0.0, N, D,
                                                                   H, None, FAKE, FAKE, None),
            ("recon", R.LIN): lambda: lib.pm_recon_exact_lin_f64(FAKE, ldy, None, FAKE, FAKE, FAKE, FAKE, K, N, D, H, FAKE,
                                                                 max(H, 1), FAKE, None),
            ("recon", R.MCA): lambda: lib.pm_recon_exact_mca_f64(FAKE, ldy, FAKE, 0.1, 0, -1.0, -0.1, 1.0, N, D, H, FAKE, ldy,
                                                                 FAKE, None),
            ("recon", R.GSC): lambda: lib.pm_recon_exact_gsc_f64(FAKE, ldy, FAKE, FAKE, FAKE, FAKE, FAKE, N, D, H, FAKE,
                                                                 max(H, 1), FAKE, None)}
        refused = 0
        for (u, k), entry in entries.items():
            want = getattr(lib, "pm_%s_exact_plan" % u)(k, N, D, K, H, out)
            if want != R.PM_OK:              # (a shape the plan accepts is not called: it would launch on the FAKE pointers)
                assert entry() == want, (u, k, N, D, K, H)
                refused += 1
        assert refused >= 1
