"""The exact-enumeration kernels (loglik_exact.hip, recon_exact.hip, pm_exact.h) through the C ABI -- pm_loglik_exact_lin_f64,
_mca_f64, _gsc_f64 and pm_recon_exact_lin_f64, _mca_f64, _gsc_f64 -- from both libraries, at the smallest shape of every
dispatch cell (each confirmed inside the test with pm_loglik_exact_plan / pm_recon_exact_plan, the host functions the
launchers themselves take their launch from), against the longdouble reference tests/exact_kernels_reference.py on the
kernels' own operands: values that are no integers (one of them 0.0), a prior row per latent, one -inf prior entry, P and G
unrelated to one another.  tests/test_exact_kernels_cpu.py pins that reference and sweeps the plans without a device.

Harness.  Y has a row stride above D, starts 8 bytes off a 16-byte boundary and carries NaN in its padding.  Outputs are
larger than needed and filled with a sentinel that must survive past the row width and past N; `work` is
work_len + 64 doubles, filled with the sentinel, whose last 64 must survive; `total` is three doubles of which one is
written.  Every loglik case runs four times -- default library; again; deterministic library under another ldy; rows_out =
NULL -- and must return the same bits each time (the NULL run through `total`), and total[0] must be, bit for bit,
total_fixed_order(rows): ex_total_kernel's order restated.  Every recon case runs four times -- default; again;
deterministic library under other strides; rows permuted -- with the same bits per row.  (The three cases at 2^32 states run
twice, default and deterministic, to stay within twice the time of test_loglik_exact_gpu.py::test_at_the_bound.)

Tolerances are the project's: loglik rows 1e-11 relative (RTOL of tests/test_loglik_exact_gpu.py), recon 1e-11 of the row's
largest entry (tests/test_reconstruct_exact_abi_gpu.py), always against the longdouble reference.  The deep cases (H = 22,
14, 8 linear with couplings across the lo / hi boundary and at the last high digit; MCA H = 20; GSC H = 14; the bounds H = 32,
20, 16) are judged by the factorised closed forms, which need no enumeration.

Worst error of each group against its bound of 1e-11 (MI355X, both libraries, the unchanged kernels; the module's autouse
fixture prints the table with -s).  Loglik: relative; recon: relative to the row's largest entry.
  lin loglik         3.0e-16  K=5 H=6 N=64          lin recon          4.6e-14  K=8 H=1 N=256
  lin depth loglik   1.3e-16  K=2 H=22 N=2          lin depth recon    2.2e-15  K=3 H=14 N=2
  lin bound loglik   1.3e-16  K=3 H=20 N=2
  mca loglik         1.9e-16  H=6 N=17 lp1=-inf     mca recon          9.7e-14  MMCA D=1024 H=3 N=2
  mca depth loglik   2.8e-16  H=20 D=20 N=32        mca depth recon    2.5e-15  MMCA H=20 D=20 N=2
  gsc loglik         2.3e-16  H=9 Lw N=63           gsc recon          2.2e-14  H=1 N=130
  gsc depth loglik   2.3e-16  H=14 wdiag N=600      gsc depth recon    8.5e-16  H=14 N=2
Every group sits two to five orders of magnitude inside the bound, at 2^32 states as at 2: DESIGN 4.13's statement that the
accuracy does not depend on the length of a range holds.  No kernel bug was found; all 75 tests pass on the unchanged kernels.

Mutants (one changed line each in a scratch copy of pm_exact.h, loglik_exact.hip or recon_exact.hip -- values, predicates and
host decisions only: no address that can leave a buffer, no loop bound that can hang --, both libraries rebuilt, this module
run once per mutant, stopping at its first failure; MI355X).  Mutant -> first failing test:
   1 pmx_lse_add: `s = s * e + 1.0` -> `s + 1.0`                      test_lin_loglik[K2_H12]  (error 1.9e-2)
   2 pmx_mca_wbar: copysign dropped from the signed power            test_mca_loglik[1-mmca]
   3 T = M_ss Lp: `p = l` -> `p = 0` (reads Lp's upper triangle)      test_gsc_loglik[5-wdiag]
   4 kappa_s: `- 0.5 * mm` -> `- mm`                                  test_gsc_loglik[1-wdiag]
   5 Cholesky update: `l <= i` -> `l < i`                             test_gsc_loglik[5-wdiag]
   6 pmx_prep_dot ignores ymu                                        test_lin_loglik[K2_H12]  (ymu given)
   7 pmx_lin_split: `<= 1024` -> `< 1024` (host)                      test_lin_loglik[K2_H12]  (the plan: L = 9, CH = 512)
   8 ex_lin g_t: `L + i` -> `L + i - 1` clamped                       test_lin_loglik[K2_H12]
   9 ex_lin packing: `3 * h` -> `2 * h`                               test_lin_loglik[K2_H12]
  10 ex_lin `>= CH` -> `> CH` in set-up and loop                     test_lin_loglik[K5_H6]   (CH = 625: lo = 625 exists; either
                                                                     line alone is equivalent: the other one discards the state)
  11 ex_lin odometer: `< K` -> `< K - 1`                              test_lin_depth_with_couplings[K2_H22]  (the shallow cases
                                                                     hold one chunk per range: R = units)
  12 ex_lin: `-0.5 * si * g` -> `-si * g`                             test_lin_loglik[K2_H12]
  13 ex_lin_tn: 64 -> 65 (host)                                      test_lin_loglik[K2_H12]  (the plan at N = 64: TN = 1)
  14 ex_combine: `+ qcoef * q` -> `- qcoef * q`                       test_lin_loglik[K2_H12]
  15 ex_total: the sums start from -0.0                              test_n_zero_writes_zero_and_nothing_else[lin]
  16 ex_gsc: `sMu[idx[i]]` -> `sMu[i]` in mu_s^T u_s                  test_gsc_loglik[5-wdiag]
  17 ex_gsc: wavefront 0 left out of the merge                       test_gsc_loglik[1-wdiag]
  18 ex_prep: Lw's diagonal skipped (`e <= d` -> `e < d`)             test_gsc_loglik[1-Lw]
  19 ex_mca: `(H - k) * lp0` without its guard                       test_mca_zero_prior[lp0-mca]  (NaN rows)
  20 block_partials: datapoint t writes the maximum of t - 1         test_lin_loglik[K2_H12]  (N = 64, the first tile of 8)
  21 rx_lin sweep 2: `sSv[i]` -> `sVal[0]`                            test_lin_recon[K2_H12]
  22 rx_lin: `sB[L + l]` -> `sB[L + l - 1]` clamped                   test_lin_recon[K2_H12]
  23 rx_mca: `lane + 64 * i` -> `lane + 32 * i`                       test_mca_recon_slabs[65-6]
  24 rx_mca: wavefront 2 added twice, 3 never                        test_mca_zero_prior[lp0-mca]  (the full state is wavefront 3's)
  25 rx_gsc: A z for A^T z                                           test_gsc_recon[5]
  26 RX_LIN_MIN_CHUNKS: 2 -> 1 (host)                                test_lin_recon[K2_H12]   (the plan: R = 4)
  27 rx_lin low latents: `& 7` -> `& 3`                               test_lin_recon[K5_H6]    (a digit of 4)
  28 lin entry: row block at `Y + n0 * D` (host)                     test_lin_recon[K2_H12]   (N = 257, under another ldy)
  29 rx_lin sweep 2: `mlo[j] += q` -> `= q`                           test_lin_recon[K2_H12]
  30 rx_combine_sum: column j takes column j - 1 (clamped)           test_lin_recon[K2_H12]
No mutant survives.  Mutants tried and dropped because they are equivalent: swapping `e / k` and `e % k` in the T product
(every (i, l) is still formed once), the dead rows of a ragged MCA tile clamped to N - 1 instead of n0 (never written), and
`lane < o` -> `lane <= o` in ex_combine's tree (lane 0 reads every partner before that partner is disturbed).

Time (MI355X, one run of the module): 75 tests in 5.0 s.  The slowest: test_lin_loglik[K2_H12] 0.38 s, test_lin_recon[K3_H8]
0.26 s, [K6_H5] 0.24 s, [K2_H12] 0.22 s, test_lin_loglik[K8_H5] 0.22 s, test_mca_depth_disjoint_supports 0.18 s; the three cases
at the bound 0.09, 0.08 and 0.06 s; every other test at most 0.13 s (most of it the longdouble reference).
"""
import ctypes
import functools

import numpy as np
import pytest

import exact_kernels_reference as R

pytestmark = pytest.mark.gpu

RTOL = 1e-11
SENT = -12345.678
LD = np.longdouble
LIN, MCA, GSC = R.LIN, R.MCA, R.GSC
KIND_NAME = {LIN: "lin", MCA: "mca", GSC: "gsc"}
WORST = {}                            # group -> (largest error, case)


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    if WORST:
        print("\nworst error per group (bound %.0e):" % RTOL)
        for g in sorted(WORST):
            print("  %-24s %.3e   %s" % (g, WORST[g][0], WORST[g][1]))


def _lib_of(det):
    from prosper_amd import _lib
    return _lib.load(det)


def _up(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _padded_y(Y, ldy, dev):
    """Y in a NaN-filled buffer with row stride ldy whose first row starts 8 bytes past a 16-byte boundary."""
    import torch
    N, D = Y.shape
    buf = torch.full((N * ldy + 3,), float("nan"), dtype=torch.float64, device=dev)
    off = 1 if buf.data_ptr() % 16 == 0 else 2
    view = buf[off:off + N * ldy].view(N, ldy)
    if N:
        view[:, :D] = torch.from_numpy(np.ascontiguousarray(Y)).to(dev)
    assert (buf.data_ptr() + 8 * off) % 16 == 8
    return buf, view, ctypes.c_void_p(buf.data_ptr() + 8 * off)


def _plan(det, unit, kind, N, D, K, H):
    out = (ctypes.c_int64 * R.PLAN_LEN)(*([-7] * R.PLAN_LEN))
    rc = getattr(_lib_of(det), "pm_%s_exact_plan" % unit)(kind, N, D, K, H, out)
    assert (rc, list(out)) == getattr(R, "%s_plan" % unit)(kind, N, D, K, H), (unit, kind, N, D, K, H, rc, list(out))
    return list(out)


def _assert_cell(unit, kind, N, D, K, H, cell):
    """Both libraries report the cell the case is meant for: `cell` maps indices of the plan's out[] to values."""
    for det in (False, True):
        p = _plan(det, unit, kind, N, D, K, H)
        for i, v in cell.items():
            assert p[i] == v, (unit, KIND_NAME[kind], N, D, K, H, "out[%d] = %d, the case is meant for %d" % (i, p[i], v), p)
    return p


# --------------------------------------------------------------------------------------------------------------- operands
NMAX = {(LIN, ""): 257, (LIN, "blocks"): 2, (LIN, "n600"): 600, (MCA, ""): 65, (MCA, "lp1"): 17, (MCA, "lp0"): 17,
        (MCA, "disjoint"): 32, (GSC, ""): 257, (GSC, "blocks"): 600, (GSC, "indef"): 3}


@functools.lru_cache(maxsize=None)
def _ops(kind, K, H, D, variant=""):
    """The operands of a case (all rows a test may ask for).  MCA: K is the `signed` flag."""
    rng = np.random.RandomState(7000 + 1000 * kind + 37 * K + H + 5 * D + sum(map(ord, variant)))
    n = NMAX[(kind, variant)]
    if kind == LIN:
        blocks = R.straddling_blocks(H, R.lin_split(K, H)[0]) if variant == "blocks" else None
        o = R.lin_operands(rng, D, H, K, n, blocks=blocks)
        o["blocks"] = blocks
    elif kind == MCA:
        o = R.mca_operands(rng, D, H, n, bool(K), disjoint=variant == "disjoint",
                           lp1=-np.inf if variant == "lp1" else np.log(0.3), lp0=-np.inf if variant == "lp0" else np.log(0.7))
    else:
        blocks = None
        if variant == "blocks":       # pairs and triples (j, j + 5, j + 10) of the 14 latents
            blocks = [[0, 5, 10], [1, 6, 11], [2, 7, 12], [3, 8, 13], [4, 9]][:5] if H == 14 else None
            assert blocks is not None
        o = R.gsc_operands(rng, D, H, n, blocks=blocks, pi_edge=variant != "indef")
        if variant == "indef":        # Psi_{0,1} past the geometric mean of the diagonal: every support with both is indefinite
            o["Psi"][0, 1] = o["Psi"][1, 0] = 3.0 * np.sqrt(o["Psi"][0, 0] * o["Psi"][1, 1])
        rng2 = np.random.RandomState(99 + H)
        o["wdiag_alt"] = rng2.uniform(0.5, 2.0, size=D)
        o["Lw_alt"] = np.tril(rng2.normal(size=(D, D)) * 0.3) + np.eye(D) + np.triu(np.full((D, D), np.nan), 1)
        o["blocks"] = blocks
    return o


def _noise(o, noise):
    return (o["wdiag_alt"] if noise == "wdiag" else None), (o["Lw_alt"] if noise == "Lw" else None)


@functools.lru_cache(maxsize=None)
def _gsc_enum(H, D, variant, n):
    o = _ops(GSC, 0, H, D, variant)
    l, kap = R._gsc_logjoint(np.asarray(o["Y"][:n], dtype=LD) @ np.asarray(o["P"], dtype=LD), o["M"], o["Psi"], o["mu"], o["logp"])
    return R.lse_rows(l)[0], R._gsc_means_from(l, kap, H)


@functools.lru_cache(maxsize=None)
def _want(unit, kind, K, H, D, variant, flag, n):
    """The reference of the first n rows.  `flag`: lin: ymu given; GSC: the noise operand."""
    o = _ops(kind, K, H, D, variant)
    Y = o["Y"][:n]
    if kind == LIN:
        a = (Y, o["ymu"] if flag else None, o["P"], o["G"], o["logp"], o["values"])
        if unit == "loglik":
            return (R.lin_block_rows(*a, o["cst"], o["qcoef"], o["blocks"]) if o["blocks"]
                    else R.lin_rows(*a, o["cst"], o["qcoef"]))
        return R.lin_block_means(*a, o["blocks"]) if o["blocks"] else R.lin_means(*a)
    if kind == MCA:
        a = (Y, o["Wrho"], o["inv_rho"], o["signed"], o["lp1"], o["lp0"], o["inv_s2"])
        if unit == "loglik":
            return R.mca_disjoint_rows(*a, o["cst"]) if variant == "disjoint" else R.mca_rows(*a, o["cst"])
        return R.mca_disjoint_means(*a) if variant == "disjoint" else R.mca_means(*a)
    wdiag, Lw = _noise(o, flag)
    if o["blocks"]:
        if unit == "loglik":
            return R.gsc_block_rows(Y, o["P"], wdiag, Lw, o["M"], o["Psi"], o["mu"], o["logp"], o["cst"], o["blocks"])
        return R.gsc_block_means(Y, o["P"], o["M"], o["Psi"], o["mu"], o["logp"], o["blocks"])
    lse, means = _gsc_enum(H, D, variant, n)
    return lse + LD(o["cst"]) - LD(0.5) * R.gsc_quad(Y, wdiag, Lw) if unit == "loglik" else means


# ---------------------------------------------------------------------------------------------------------------- runners
def _loglik(dev, det, kind, o, N, ldy, flag, give_rows=True):
    """One call of the kind's loglik entry on guarded buffers: (rows or None, total bits as float64)."""
    import torch
    lib = _lib_of(det)
    Y = o["Y"][:N]
    D = Y.shape[1]
    H = o["logp"].shape[0] if kind != MCA else o["Wrho"].shape[0]
    keep, _, yp = _padded_y(Y, ldy, dev)
    wl = int(lib.pm_loglik_exact_work_len(N, H))
    assert wl >= 1
    work = torch.full((wl + 64,), SENT, dtype=torch.float64, device=dev)
    rows = torch.full((N + 5,), SENT, dtype=torch.float64, device=dev)
    total = torch.full((3,), SENT, dtype=torch.float64, device=dev)
    rp = _ptr(rows) if give_rows else None
    dbl = ctypes.c_double
    if kind == LIN:
        d = {k: _up(o[k], dev) for k in ("P", "G", "logp", "values")}
        mu = _up(o["ymu"], dev) if flag else None
        rc = lib.pm_loglik_exact_lin_f64(yp, ldy, _ptr(mu), _ptr(d["P"]), _ptr(d["G"]), _ptr(d["logp"]), _ptr(d["values"]),
                                         o["K"], dbl(o["cst"]), dbl(o["qcoef"]), N, D, H, rp, _ptr(work), _ptr(total), None)
    elif kind == MCA:
        d = {"Wrho": _up(o["Wrho"], dev)}
        rc = lib.pm_loglik_exact_mca_f64(yp, ldy, _ptr(d["Wrho"]), dbl(o["inv_rho"]), o["signed"], dbl(o["lp1"]), dbl(o["lp0"]),
                                         dbl(o["inv_s2"]), dbl(o["cst"]), N, D, H, rp, _ptr(work), _ptr(total), None)
    else:
        d = {k: _up(o[k], dev) for k in ("P", "M", "Psi", "mu", "logp")}
        wdiag, Lw = _noise(o, flag)
        wd, lw = (None if wdiag is None else _up(wdiag, dev)), (None if Lw is None else _up(Lw, dev))
        rc = lib.pm_loglik_exact_gsc_f64(yp, ldy, _ptr(d["P"]), _ptr(wd), _ptr(lw), _ptr(d["M"]), _ptr(d["Psi"]), _ptr(d["mu"]),
                                         _ptr(d["logp"]), dbl(o["cst"]), N, D, H, rp, _ptr(work), _ptr(total), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((work[wl:] == SENT).all()), "the tail past pm_loglik_exact_work_len was written"
    assert bool((total[1:] == SENT).all()), "total[1:] was written"
    if N == 0:
        assert bool((work == SENT).all()), "N = 0 wrote to work"
    if give_rows:
        assert bool((rows[N:] == SENT).all()), "rows past N were written"
    else:
        assert bool((rows == SENT).all())
    return (rows[:N].cpu().numpy() if give_rows else None), total[:1].cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b, what):
    assert np.array_equal(_bits(a), _bits(b)), what


def _loglik_all(dev, kind, o, N, flag, cell, K=0, runs=4):
    """The four runs of a loglik case (module docstring); returns the rows."""
    D = o["Y"].shape[1]
    H = o["logp"].shape[0] if kind != MCA else o["Wrho"].shape[0]
    _assert_cell("loglik", kind, N, D, K, H, cell)
    rows, total = _loglik(dev, False, kind, o, N, D + 3, flag)
    assert _bits(total)[0] == _bits([R.total_fixed_order(rows)])[0], ("total is not the fixed-order sum of the rows", N)
    rows_d, total_d = _loglik(dev, True, kind, o, N, D + 1, flag)
    _same(rows, rows_d, "rows: deterministic library, other ldy")
    _same(total, total_d, "total: deterministic library, other ldy")
    if runs == 4:
        rows_2, total_2 = _loglik(dev, False, kind, o, N, D + 3, flag)
        _same(rows, rows_2, "rows: second call")
        _same(total, total_2, "total: second call")
        _, total_n = _loglik(dev, False, kind, o, N, D + 3, flag, give_rows=False)
        _same(total, total_n, "total with rows_out = NULL")
    return rows


def _recon(dev, det, kind, o, N, ldy, ldo, extra_rows, flag, perm=None):
    """One call of the kind's recon entry on guarded buffers: the (N, width) result."""
    import torch
    lib = _lib_of(det)
    Y = o["Y"][:N]
    if perm is not None:
        Y = Y[perm]
    D = Y.shape[1]
    H = o["logp"].shape[0] if kind != MCA else o["Wrho"].shape[0]
    width = D if kind == MCA else H
    keep, _, yp = _padded_y(Y, ldy, dev)
    wl = int(lib.pm_recon_exact_work_len(N, H, D))
    assert wl >= 1
    work = torch.full((wl + 64,), SENT, dtype=torch.float64, device=dev)
    out = torch.full((N + extra_rows, ldo), SENT, dtype=torch.float64, device=dev)
    dbl = ctypes.c_double
    if kind == LIN:
        d = {k: _up(o[k], dev) for k in ("P", "G", "logp", "values")}
        mu = _up(o["ymu"], dev) if flag else None
        rc = lib.pm_recon_exact_lin_f64(yp, ldy, _ptr(mu), _ptr(d["P"]), _ptr(d["G"]), _ptr(d["logp"]), _ptr(d["values"]), o["K"],
                                        N, D, H, _ptr(out), ldo, _ptr(work), None)
    elif kind == MCA:
        d = {"Wrho": _up(o["Wrho"], dev)}
        rc = lib.pm_recon_exact_mca_f64(yp, ldy, _ptr(d["Wrho"]), dbl(o["inv_rho"]), o["signed"], dbl(o["lp1"]), dbl(o["lp0"]),
                                        dbl(o["inv_s2"]), N, D, H, _ptr(out), ldo, _ptr(work), None)
    else:
        d = {k: _up(o[k], dev) for k in ("P", "M", "Psi", "mu", "logp")}
        rc = lib.pm_recon_exact_gsc_f64(yp, ldy, _ptr(d["P"]), _ptr(d["M"]), _ptr(d["Psi"]), _ptr(d["mu"]), _ptr(d["logp"]), N,
                                        D, H, _ptr(out), ldo, _ptr(work), None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((work[wl:] == SENT).all()), "the tail past pm_recon_exact_work_len was written"
    full = out.cpu().numpy()
    assert np.all(full[:N, width:] == SENT), "columns past the row width were written"
    assert np.all(full[N:] == SENT), "rows past N were written"
    return np.ascontiguousarray(full[:N, :width])


def _recon_all(dev, kind, o, N, flag, cell, K=0):
    """The four runs of a recon case (module docstring); returns the (N, width) result."""
    D = o["Y"].shape[1]
    H = o["logp"].shape[0] if kind != MCA else o["Wrho"].shape[0]
    width = D if kind == MCA else H
    _assert_cell("recon", kind, N, D, K, H, cell)
    got = _recon(dev, False, kind, o, N, D + 3, width + 2, 3, flag)
    _same(got, _recon(dev, False, kind, o, N, D + 3, width + 2, 3, flag), "second call")
    _same(got, _recon(dev, True, kind, o, N, D + 1, width, 0, flag), "deterministic library, other strides")
    perm = np.random.RandomState(N).permutation(N)
    _same(got[perm], _recon(dev, False, kind, o, N, D + 2, width + 1, 1, flag, perm=perm), "rows permuted")
    return got


def _note(group, err, case):
    if group not in WORST or err > WORST[group][0]:
        WORST[group] = (err, case)


def _check_rows(group, case, got, want):
    want = np.asarray(want, dtype=LD)
    assert got.shape == want.shape and np.isfinite(want).all() and np.isfinite(got).all(), (case, got, want)
    err = float(np.max(np.abs(got.astype(LD) - want) / np.abs(want)))
    _note(group, err, case)
    print("%-22s %-34s relative error %.3e (bound %.0e)" % (group, case, err, RTOL))
    assert err <= RTOL, (group, case, err)


def _check_recon(group, case, got, want):
    want = np.asarray(want, dtype=LD)
    assert got.shape == want.shape and np.isfinite(want).all() and np.isfinite(got).all(), (case, got, want)
    scale = np.abs(want).max(axis=1)
    err = float((np.abs(got.astype(LD) - want).max(axis=1) / np.where(scale > 0, scale, LD(1))).max())
    _note(group, err, case)
    print("%-22s %-34s error relative to the row's largest entry %.3e (bound %.0e)" % (group, case, err, RTOL))
    assert err <= RTOL, (group, case, err)


# ---------------------------------------------------------------------------------------------------------- linear models
LIN_IDS = ["K%d_H%d" % kh for kh in R.LIN_CELLS]


@pytest.mark.parametrize("K,H", list(R.LIN_CELLS), ids=LIN_IDS)
def test_lin_loglik(dev, K, H):
    """K = 2..8 with two high digits (CH = 1024, 729, 1024, 625, 216, 343, 512: threads without a lo state, last lo slots
    that only some threads own, digits of 7) and H <= L (one chunk, NH = 0); N on both sides of the tile switch at 64 with
    ragged last tiles; ymu given and NULL."""
    L, CH, chunks = R.LIN_CELLS[(K, H)]
    o = _ops(LIN, K, H, 5)
    assert 0.0 in o["values"] and np.isinf(o["logp"]).sum() == 1 and not np.all(o["values"] == np.round(o["values"]))
    nmax = max(R.LIN_LOGLIK_N)
    for i, N in enumerate(R.LIN_LOGLIK_N):
        flag = i % 2 == 0
        cell = {0: 8 if N >= 64 else 1, 1: L, 2: CH, 3: chunks, 5: min(chunks, -(-4096 // -(-N // (8 if N >= 64 else 1))))}
        rows = _loglik_all(dev, LIN, o, N, flag, cell, K=K)
        _check_rows("lin loglik", "K=%d H=%d N=%d ymu=%d" % (K, H, N, flag), rows, _want("loglik", LIN, K, H, 5, "", flag, nmax)[:N])


@pytest.mark.parametrize("K,H", list(R.LIN_CELLS), ids=LIN_IDS)
def test_lin_recon(dev, K, H):
    """The same cells through both sweeps of rx_lin_kernel; N around the 256-row block of the host walk where the state
    count keeps the reference small (K^H <= 8192), else N = 1 and 7."""
    L, CH, chunks = R.LIN_CELLS[(K, H)]
    o = _ops(LIN, K, H, 5)
    Ns = R.LIN_RECON_N if K ** H <= 8192 else (1, 7)
    for i, N in enumerate(Ns):
        flag = i % 2 == 1
        cell = {0: 256, 1: -(-N // 256), 2: L, 3: CH, 4: chunks, 5: max(1, chunks // 2)}
        got = _recon_all(dev, LIN, o, N, flag, cell, K=K)
        _check_recon("lin recon", "K=%d H=%d N=%d ymu=%d" % (K, H, N, flag), got, _want("recon", LIN, K, H, 5, "", flag, max(Ns))[:N])


@pytest.mark.parametrize("K,H", list(R.LIN_DEPTH), ids=["K%d_H%d" % kh for kh in R.LIN_DEPTH])
def test_lin_depth_with_couplings(dev, K, H):
    """NH = 12, 8 and 5 high digits with G non-zero inside blocks of 2 and 3 latents that straddle the lo / hi boundary, among
    them {L-1, L, H-1}: G_lh and G_hh at the last high digit, the odometer's carries, sB[L + l] -- what W = 0 cannot see.
    Judged by the factorised closed form."""
    L, CH, chunks, r_ll, r_rx = R.LIN_DEPTH[(K, H)]
    o = _ops(LIN, K, H, 5, "blocks")
    assert [L - 1, L, H - 1] in o["blocks"] and o["G"][L - 1, H - 1] != 0 and o["G"][L, H - 1] != 0
    rows = _loglik_all(dev, LIN, o, 2, True, {0: 1, 1: L, 2: CH, 3: chunks, 5: r_ll}, K=K)
    _check_rows("lin depth loglik", "K=%d H=%d N=2" % (K, H), rows, _want("loglik", LIN, K, H, 5, "blocks", True, 2))
    got = _recon_all(dev, LIN, o, 2, True, {2: L, 3: CH, 4: chunks, 5: r_rx}, K=K)
    _check_recon("lin depth recon", "K=%d H=%d N=2" % (K, H), got, _want("recon", LIN, K, H, 5, "blocks", True, 2))


@pytest.mark.parametrize("K,H", list(R.LIN_BOUND), ids=["K%d_H%d" % kh for kh in R.LIN_BOUND])
def test_lin_loglik_at_the_bound_with_couplings(dev, K, H):
    """2^32 states (3^20 for K = 3) with the same straddling blocks, N = 2, two runs (default and deterministic library).
    Measured against tests/test_loglik_exact_gpu.py::test_at_the_bound of the same H in the same session (MI355X): K = 2, H = 32
    0.09 s against 0.19 s [bsc]; K = 3, H = 20 0.08 s against 0.06 s [tsc]; K = 4, H = 16 0.06 s against 0.05 s [dsc4]: all
    three inside twice the existing case, so all three bounds are kept."""
    L, CH, chunks, r_ll = R.LIN_BOUND[(K, H)]
    o = _ops(LIN, K, H, 5, "blocks")
    rows = _loglik_all(dev, LIN, o, 2, False, {0: 1, 1: L, 2: CH, 3: chunks, 5: r_ll}, K=K, runs=2)
    _check_rows("lin bound loglik", "K=%d H=%d N=2" % (K, H), rows, _want("loglik", LIN, K, H, 5, "blocks", False, 2))


# ------------------------------------------------------------------------------------------------------------ MCA / MMCA
@pytest.mark.parametrize("signed", [0, 1], ids=["mca", "mmca"])
@pytest.mark.parametrize("H", R.MCA_H)
def test_mca_loglik(dev, H, signed):
    """H = 1, 6 (one range), 11 (two); N on both sides of the tile switch at 16 with a ragged last tile; MMCA: sums over the
    causes that cross zero."""
    o = _ops(MCA, signed, H, 7)
    if signed and H >= 2:
        assert (o["Wrho"][0, 0] + o["Wrho"][1, 0]) * o["Wrho"][0, 0] < 0
    for N in R.MCA_LOGLIK_N:
        cell = {0: 4 if N >= 16 else 1, 3: 1 << H, 5: 2 if H == 11 else 1}
        rows = _loglik_all(dev, MCA, o, N, None, cell)
        _check_rows("mca loglik", "signed=%d H=%d N=%d" % (signed, H, N), rows,
                    _want("loglik", MCA, signed, H, 7, "", None, max(R.MCA_LOGLIK_N))[:N])


@pytest.mark.parametrize("signed", [0, 1], ids=["mca", "mmca"])
@pytest.mark.parametrize("edge", ["lp1", "lp0"])
def test_mca_zero_prior(dev, edge, signed):
    """lp1 = -inf leaves the empty state alone, lp0 = -inf the full one: the `k ? ... : 0.0` guards of both units."""
    o = _ops(MCA, signed, 6, 7, edge)
    assert o[edge] == -np.inf
    rows = _loglik_all(dev, MCA, o, 17, None, {0: 4, 3: 64, 5: 1})
    _check_rows("mca loglik", "signed=%d H=6 N=17 %s=-inf" % (signed, edge), rows, _want("loglik", MCA, signed, 6, 7, edge, None, 17))
    got = _recon_all(dev, MCA, o, 3, None, {0: 64, 1: 1, 5: 1, 6: 1})
    want = _want("recon", MCA, signed, 6, 7, edge, None, 3)
    if edge == "lp1":
        assert np.all(got == 0.0) and np.all(want == 0)          # Wbar(0) = 0 carries all the weight
    else:
        _check_recon("mca recon", "signed=%d H=6 N=3 lp0=-inf" % signed, got, want)


@pytest.mark.parametrize("signed", [0, 1], ids=["mca", "mmca"])
@pytest.mark.parametrize("H", R.MCA_H)
def test_mca_recon_rows(dev, H, signed):
    """H = 1, 6, 11 (R = 1, 1, 32); at H = 6 N around the 64-row block of the host walk."""
    o = _ops(MCA, signed, H, 5)
    Ns = (1,) + R.MCA_RECON_N if H == 6 else (1, 3)
    for N in Ns:
        got = _recon_all(dev, MCA, o, N, None, {0: 64, 1: -(-N // 64), 4: 1 << H, 5: {1: 1, 6: 1, 11: 32}[H], 6: 1})
        _check_recon("mca recon", "signed=%d H=%d N=%d" % (signed, H, N), got, _want("recon", MCA, signed, H, 5, "", None, max(Ns))[:N])


@pytest.mark.parametrize("D,H", [(D, 6) for D in R.MCA_RECON_D] + [(1024, 3)])
def test_mca_recon_slabs(dev, D, H):
    """The 64-wide slabs of the dimensions: D = 1, 63, 64, 65, 128 and the bound 1024 (16 slabs)."""
    signed = int(D % 2 == 0)
    o = _ops(MCA, signed, H, D)
    N = 2 if D == 1024 else 3
    got = _recon_all(dev, MCA, o, N, None, {6: -(-D // 64), 5: 1})
    _check_recon("mca recon", "signed=%d D=%d H=%d N=%d" % (signed, D, H, N), got, _want("recon", MCA, signed, H, D, "", None, N))


def test_mca_recon_refuses_d_1025(dev):
    import torch
    D, H, N = 1025, 3, 2
    for det in (False, True):
        lib = _lib_of(det)
        Y = torch.zeros((N, D), dtype=torch.float64, device=dev)
        W = torch.ones((H, D), dtype=torch.float64, device=dev)
        out = torch.full((N, D), SENT, dtype=torch.float64, device=dev)
        work = torch.full((int(lib.pm_recon_exact_work_len(N, H, D)),), SENT, dtype=torch.float64, device=dev)
        rc = lib.pm_recon_exact_mca_f64(_ptr(Y), D, _ptr(W), 0.1, 0, -1.0, -0.3, 1.0, N, D, H, _ptr(out), D, _ptr(work), None)
        torch.cuda.synchronize()
        assert rc == R.PM_ERANGE and bool((out == SENT).all()) and bool((work == SENT).all())
        out64 = (ctypes.c_int64 * R.PLAN_LEN)()
        assert lib.pm_recon_exact_plan(MCA, N, D, 0, H, out64) == R.PM_ERANGE


def test_mca_depth_disjoint_supports(dev):
    """H = 20, D = 20, every dimension owned by one cause: 2^20 states against the closed form, loglik at N = 2 (R = units =
    1024) and N = 32 (tiles of 4, 1 < R = 512 < units), recon at N = 2 (R = 64, the cap)."""
    for signed in (0, 1):
        o = _ops(MCA, signed, 20, 20, "disjoint")
        for N, Rr in ((2, 1024), (32, 512)):
            rows = _loglik_all(dev, MCA, o, N, None, {0: 4 if N >= 16 else 1, 3: 1 << 20, 4: 1024, 5: Rr})
            _check_rows("mca depth loglik", "signed=%d H=20 D=20 N=%d" % (signed, N), rows,
                        _want("loglik", MCA, signed, 20, 20, "disjoint", None, 32)[:N])
        got = _recon_all(dev, MCA, o, 2, None, {4: 1 << 20, 5: 64, 6: 1})
        _check_recon("mca depth recon", "signed=%d H=20 D=20 N=2" % signed, got, _want("recon", MCA, signed, 20, 20, "disjoint", None, 32)[:2])


# -------------------------------------------------------------------------------------------------------------------- GSC
@pytest.mark.parametrize("noise", ["wdiag", "Lw", "none"])
@pytest.mark.parametrize("H", R.GSC_H)
def test_gsc_loglik(dev, H, noise):
    """H = 1, 5 (one range), 9 (16 ranges = units); wdiag, Lw (its strict upper triangle NaN: never read) and neither; N around
    the 64-lane tile; one pi_h = 0 and one pi_h = 1 (H >= 3)."""
    o = _ops(GSC, 0, H, 5)
    assert np.isinf(o["logp"]).sum() == (2 if H >= 3 else 0)
    for N in R.GSC_N:
        rows = _loglik_all(dev, GSC, o, N, noise, {0: 64, 3: 1 << H, 5: {1: 1, 5: 1, 9: 16}[H], 6: -(-N // 64) * {1: 1, 5: 1, 9: 16}[H]})
        _check_rows("gsc loglik", "H=%d %s N=%d" % (H, noise, N), rows, _want("loglik", GSC, 0, H, 5, "", noise, 257)[:N])


@pytest.mark.parametrize("H", R.GSC_H)
def test_gsc_recon(dev, H):
    """... and both sweeps of rx_gsc_kernel; at H = 5 also N = 257, a second row block."""
    o = _ops(GSC, 0, H, 5)
    for N in R.GSC_N + ((257,) if H == 5 else ()):
        got = _recon_all(dev, GSC, o, N, None, {0: 256, 1: -(-N // 256), 4: 1 << H, 5: {1: 1, 5: 1, 9: 16}[H]})
        _check_recon("gsc recon", "H=%d N=%d" % (H, N), got, _want("recon", GSC, 0, H, 5, "", None, 257)[:N])
        if H >= 3:
            assert np.all(got[:, 1] == 0.0)                      # pi_1 = 0


def test_gsc_indefinite_psi_block(dev):
    """Psi_{0,1} makes every support that holds latents 0 and 1 indefinite: those terms are NaN, so every row is."""
    o = _ops(GSC, 0, 5, 5, "indef")
    want = _want("loglik", GSC, 0, 5, 5, "indef", "none", 3)
    assert np.isnan(want).all()
    for det in (False, True):
        rows, total = _loglik(dev, det, GSC, o, 3, 8, "none")
        assert np.isnan(rows).all() and np.isnan(total).all()
        assert np.isnan(_recon(dev, det, GSC, o, 3, 8, 7, 2, None)).all()


def test_gsc_depth_block_diagonal(dev):
    """H = 14, M and Psi block-diagonal in pairs and triples (j, j + 5, j + 10): supports of up to 14 latents against the
    closed form.  Loglik at N = 2 (R = units = 512) and N = 600 (10 tiles, 1 < R = 410 < units), recon at N = 2 (R = 256, the cap)."""
    o = _ops(GSC, 0, 14, 5, "blocks")
    for N, Rr, noise in ((2, 512, "Lw"), (600, 410, "wdiag")):
        rows = _loglik_all(dev, GSC, o, N, noise, {0: 64, 3: 1 << 14, 4: 512, 5: Rr})
        _check_rows("gsc depth loglik", "H=14 %s N=%d" % (noise, N), rows, _want("loglik", GSC, 0, 14, 5, "blocks", noise, 600)[:N])
    got = _recon_all(dev, GSC, o, 2, None, {4: 1 << 14, 5: 256})
    _check_recon("gsc depth recon", "H=14 N=2", got, _want("recon", GSC, 0, 14, 5, "blocks", None, 2))


# ------------------------------------------------------------------------------------------------------------ range cells
def test_range_cells(dev):
    """One case per kind and unit with R = 1, with R at its cap by the units (loglik; in recon_exact.hip that is the single
    chunk, R = 1) and with 1 < R < cap, named by the plan.  The cases run in the tests above (the same (kind, N, K, H)): here
    every literal is held against both libraries' plans.  No valid input has a range with c0 == c1
    (tests/test_exact_kernels_cpu.py::test_no_range_is_empty)."""
    for (unit, kind, N, K, H), (Rr, cap) in R.RANGE_CELLS.items():
        _assert_cell(unit, kind, N, 20 if kind == MCA else 5, K, H, {5: Rr, 4: cap})


# ---------------------------------------------------------------------------------------------------------- loglik outputs
@pytest.mark.parametrize("N", [1, 255, 256, 257, 600])
def test_total_is_the_fixed_order_sum_of_the_rows(dev, N):
    """total[0] against ex_total_kernel's order restated (one strided pass of 256 threads, then the tree), around one pass of
    the threads and at N = 600; rows_out NULL and given, both libraries: inside _loglik_all."""
    o = _ops(LIN, 2, 3, 5, "n600")
    rows = _loglik_all(dev, LIN, o, N, True, {1: 3, 2: 8, 3: 1, 5: 1}, K=2)
    _check_rows("lin loglik", "K=2 H=3 N=%d (total)" % N, rows, R.lin_rows(o["Y"][:N], o["ymu"], o["P"], o["G"], o["logp"], o["values"],
                                                                            o["cst"], o["qcoef"]))


@pytest.mark.parametrize("kind", [LIN, MCA, GSC], ids=["lin", "mca", "gsc"])
def test_n_zero_writes_zero_and_nothing_else(dev, kind):
    import torch
    o = _ops(kind, 2 if kind == LIN else 0, 3 if kind == LIN else 5, 5)
    for det in (False, True):
        rows, total = _loglik(dev, det, kind, o, 0, 8, "none" if kind == GSC else True)          # (asserts work, rows, total[1:])
        assert rows.shape == (0,) and _bits(total)[0] == 0                                        # +0.0
        assert _recon(dev, det, kind, o, 0, 8, 9, 2, True).shape[0] == 0                          # (asserts out and work's tail)
    torch.cuda.synchronize()
