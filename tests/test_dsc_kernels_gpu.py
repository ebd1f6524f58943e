"""The DSC / TSC kernels (dsc_kernels.hip, and the fused selection of bsc_rows16.hip) through the C ABI --
pm_dsc_estep_f64, pm_dsc_estep_mstats_f64, pm_dsc_mstep_rows_f64 / _nz_f64 / _cutp_f64, pm_dsc_select_scores_f64,
pm_tsc_select_scores_f64, pm_xsc_select_f64 -- on padded, guarded operands, one smallest shape per dispatch cell (confirmed
with pm_dsc_plan inside the test), against the plain NumPy reference tests/dsc_kernels_reference.py, from both libraries.

Harness: ``Emb`` of tests/test_eval_kernels_gpu.py (16 guard rows before and after, padding columns, a quiet-NaN payload /
0xDEADBEEF / 0xA5 pattern; here also 0xA5A5 for the uint16 lists).  After every call the result block equals the reference,
every guard and padding element of every output still holds the pattern, every input is bit-unchanged.  The uint8 state
table and the int32 candidates start at odd element offsets; scores, log-joints and E[s] rows have padded leading dimensions.

Exact arithmetic.  Scores, Gram entries, |y|^2 and the latent values are small integers, ecoef is -2 or -2^-20, pscale 1 or
1/2, the prior a multiple of 2^-4: every energy is an integer far below 2^53 and ecoef e + pscale prior is exact with or
without a fused multiply-add, on the table path and on the generic walk (tests/test_dsc_kernels_cpu.py asserts it for every
case).  Log-joints, selection scores, candidates (ties are real ties) and the zero rows of cut datapoints are compared with
equality.

The bound on lse = m + log(sum_k exp(f_k - m)), derived.  u = 2^-53.  f_k - m is exact (multiples of 2^-20 below 2^17).
pm_exp_tab documents 2.3e-16 relative error per term.  A lane adds at most ceil(Kt / 16) terms one after the other, the row
is then summed in 4 steps (16 lanes; 6 for a wavefront, which has fewer terms per lane): every partial sum rounds once, so the
sum carries at most 2.3e-16 + (ceil(Kt / 16) + 6) u relative error.  Terms below e^-37 of the largest are dropped: at most
Kt e^-37 relative to a sum >= 1.  log(sum), with sum in [1, Kt], turns a relative error of its argument into an absolute one
and adds its own rounding, at most 2 ulp of a value <= max(1, log Kt): 4 u max(1, log Kt).  The final addition rounds to
u |lse|, the reference's cast to float64 another u |lse|.  The rounding part is applied with a factor 4:
    |lse - ref| <= 4 (2.3e-16 + (ceil(Kt / 16) + 6) u + 4 u max(1, log Kt) + 2 u |lse|) + Kt e^-37
(dsc_kernels_reference.lse_bound).

Posterior-weighted outputs (E[s] rows, Wq, qdiag, the value counts, sum q e) use the 1e-11 row-relative bound of
tests/test_eval_kernels_gpu.py against the longdouble reference (statistics: relative to the largest stored value of their
section).  The reference leaves out the weights the kernels document as left out (below e^-37 of a row's largest term in the
one-pass statistics, below e^-60 of the evidence in the row pass; exact operands, so both sides take the same decisions):
a row whose whole expectation lies below the cut-off is then zero on both sides.  Such a bound cannot see a state of weight
1e-12, so every case also runs HOT: ecoef = -2^-20 and a flat prior put all weights of a row within a factor e, and a
dropped, doubled or misplaced column moves a result by ~1 / Kt.  The COLD run (ecoef = -2) has terms below the e^-37 /
e^-60 cut-offs.

Deterministic library: quanta for unit `dsc` are installed as det_quanta of tests/test_dense_kernels_gpu.py does for `gemm`.
The bound 2^k >= 4 N max(|e|, |lse|, H'^2 v^2) exceeds every partial sum; the quantum is 2^(k - 51).  Integer outputs (kept,
overflow) are not quantised.  A statistic receives at most N + 1 quantised addends (one per datapoint for Wq and qdiag, one
per wavefront for counts and scalars), each off by at most quantum / 2: the bound widens by (N + 1) quantum / 2.

Mutants of dsc_kernels.hip (values and predicates only) and the check that fails on each, default library, MI355X:
  lse cut `>` -> `>=`                      32 tests: "cut rows are not zero" (the datapoint whose lse equals the cut)
  `2.0 * v[k] * s_G` -> `1.0 *`            5: logpj of km8_nt_over, km8_16_16, k8, too_many, too_many_wave (the generic walk)
  `DSC_TERM_CUT = -37.0` -> `-3.0`         32: lse of the cold runs
  pscale ignored in the states' columns    31: logpj of the cold runs (pscale = 1/2)
  lastmask always all-ones                 4: E[s] rows and Wq of tsc_l16, tsc_l16_16, tsc_wave
  `c2 = -2.0 * v` -> `+2.0 * v`            26: logpj of every case with energy-term tables
  K0 counted among the values              27: "an entry no datapoint contributes to was written" (counts[K0])"""
import ctypes
import functools

import numpy as np
import pytest

import dsc_kernels_reference as R
from test_eval_kernels_gpu import GUARD_ROWS, LAYOUTS, RTOL, Emb as _Emb, _ld, _stream, dev, row_rel  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT_U16 = 0xA5A5 - 0x10000
PM_OK, PM_EINVAL, PM_ERANGE = 0, -1, -2
LD = np.longdouble
CASE_NAMES = list(R.CASES)


class Emb(_Emb):
    """... and uint16 (the non-zero lists), carried as int16."""
    _TYPES = dict(_Emb._TYPES)
    _TYPES[np.dtype(np.uint16)] = (torch.int16, SENT_U16)

    def host_u16(self):
        return self.host().view(np.uint16)


def _odd(array, ld, dev, fill=True):
    """An operand that starts at an odd element offset of its buffer."""
    e = Emb(array, ld, dev, off=1 if (GUARD_ROWS * ld) % 2 == 0 else 2, fill=fill)
    assert e.start % 2 == 1
    return e


def _params(c, **over):
    from prosper_amd import _lib
    P = _lib.DscParams()
    P.K, P.K0 = c["K"], c["K0"]
    for k in range(c["K"]):
        P.values[k] = c["values"][k]
        P.logpi[k] = -0.25 * (k + 1)
    P.pre1, P.ecoef, P.pscale, P.flags = -0.125, c["ecoef"], c["pscale"], c["flags"]
    for k, v in over.items():
        setattr(P, k, v)
    return P


def _lib_of(det):
    from prosper_amd import _lib
    return _lib.load(det)


def _plan(det, which, c):
    out = (ctypes.c_int32 * 8)(*([-7] * 8))
    rc = _lib_of(det).pm_dsc_plan(which, c["H"], c["Hp"], c["S"], c["K"], c["flags"], c["N"], out)
    return rc, tuple(out)


@functools.lru_cache(maxsize=None)
def _case(name, hot):
    """Operands and reference of a case, computed once and shared by every test (and both libraries)."""
    c = R.make_case(name, hot)
    ref = R.case_reference(c)
    assert ref["exact"]
    return c, ref


def _inputs(dev, c, layout):
    H, Hp, S, N = c["H"], c["Hp"], c["S"], c["N"]
    ops = dict(A=Emb(c["A"], _ld(H, layout, 0), dev), G=Emb(c["G"], H, dev), yn=Emb(c["yn"], N, dev),
               cand=_odd(c["cand"], Hp, dev), prior=Emb(c["prior"], c["Kt"], dev))
    ops["tab"] = _odd(c["state_idx"], Hp, dev) if S else None
    return ops


def _tabptr(ops):
    return ops["tab"].ptr if ops["tab"] is not None else None


def _unchanged(ops):
    return all(e.unchanged() for e in ops.values() if e is not None)


def _install_quanta(c, ref):
    """Quanta of unit `dsc` in the deterministic library (module docstring); returns the quantum."""
    from prosper_amd import _lib
    from prosper_amd.em.camodels import _device
    big = max(float(np.abs(ref["E"][:c["rows"]]).max()), float(np.abs(ref["lse"][:c["rows"]]).max()),
              c["Hp"] ** 2 * float(np.abs(c["values"]).max()) ** 2, 1.0)
    k = int(np.ceil(np.log2(4.0 * c["N"] * big)))
    M8 = (ctypes.c_double * 8)(*([1.5 * 2.0 ** (k + 1)] * 8))
    _device._DET_QUANTA_SET.pop("dsc", None)
    _lib.call("pm_det_set_quanta", _lib.DET_UNITS["dsc"], M8, _stream(), det=True)
    torch.cuda.synchronize()
    return 2.0 ** (k - 51)


def _sections(H, D):
    o = H * D
    return dict(Wp=slice(0, o), Wq=slice(o, o + H * H), qdiag=slice(o + H * H, o + H * H + H),
                counts=slice(o + H * H + H, o + H * H + H + R.MAX_K), sig=slice(o + H * H + H + R.MAX_K, o + H * H + H + R.MAX_K + 1),
                lse=slice(o + H * H + H + R.MAX_K + 1, o + H * H + H + R.MAX_K + 2))


def _stats_start(H, D):
    """A non-zero start the statistics are accumulated into: position-dependent multiples of 1/8 in [1/8, 1]."""
    n = R.stats_len(H, D)
    return (1 + (np.arange(n) * 5) % 8) / 8.0


def _check_stats(got, start, want, H, D, N, widen, what):
    total = start.astype(LD) + want
    assert np.array_equal(got[:H * D], start[:H * D]), (what, "Wp section written")
    zero = np.asarray(want == 0)
    assert np.array_equal(got[zero], start[zero]), (what, "an entry no datapoint contributes to was written",
                                                    np.nonzero(got[zero] != start[zero])[0][:5].tolist())
    for sec, sl in _sections(H, D).items():
        scale = float(np.abs(total[sl]).max())
        err = float(np.abs(got[sl].astype(LD) - total[sl]).max())
        assert err <= RTOL * scale + widen, (what, sec, err, scale)
    assert got[-2] == float(total[-2]) and got[-1] == float(total[-1]), (what, "kept / overflow", got[-2:], total[-2:])


def _check_lists(idx, val_emb, expect, keep, overflow_got, overflow_start, what):
    """The lists against the E[s] rows the SAME call returned, exactly: the ascending non-zero latents of a row, the first
    PM_BSC_NZ_MAX kept, 0xFFFF in the other index slots, the other value slots never written; the overflow count.  Returns
    the non-zero counts."""
    N = expect.shape[0]
    val = val_emb.host()
    raw = val_emb.block().contiguous().view(torch.int64).cpu().numpy()
    nzm = expect != 0
    counts = nzm.sum(axis=1)
    rank = np.cumsum(nzm, axis=1) - 1
    n_i, h_i = np.nonzero(nzm)
    r_i = rank[n_i, h_i]
    sel = r_i < R.NZ_MAX
    want_idx = np.full((N, R.NZ_MAX), R.NZ_PAD, dtype=np.int64)
    want_idx[n_i[sel], r_i[sel]] = h_i[sel]
    filled = want_idx != R.NZ_PAD
    assert np.array_equal(idx.astype(np.int64), want_idx), (what, "nz_idx", np.argwhere(idx != want_idx)[:5].tolist())
    assert np.array_equal(val[filled], expect[n_i[sel], h_i[sel]]), (what, "nz_val")
    assert (raw[~filled] == val_emb.sent).all(), (what, "nz_val written behind the list")
    over = int((keep & (counts > R.NZ_MAX)).sum())
    assert overflow_got - overflow_start == over, (what, overflow_got, over)
    return counts


def _mult(c, keep_rows):
    """Datapoints per distinct row of a (periodic) case."""
    return np.bincount(np.arange(c["N"]) % c["rows"], minlength=c["rows"])


def _ref_rows(c, ref, lse_in, cut, onepass=False):
    """Reference of the row pass on the distinct rows, tiled: (expect (N, H), stats, keep (N,), nz counts (N,)).  Weights
    the kernels document as left out count as zero: below e^-37 of the row's largest log-joint in the one-pass statistics,
    below e^-60 of the evidence in the row pass (the differences are formed from exact float64 operands, so the reference
    takes the same decisions)."""
    r = c["rows"]
    with np.errstate(invalid="ignore"):
        keep = np.asarray(lse_in[:r] > cut)
    F64 = ref["F64"][:r]
    drop = R.dropped_below(F64, F64.max(axis=1), -37.0) if onepass else \
        R.dropped_below(F64, np.asarray(lse_in[:r], dtype=np.float64), -60.0)
    st = R.row_stats(ref["F64"][:r], np.where(keep, lse_in[:r], 0.0), keep, ref["E"][:r], c["cand"][:r], c["values"], c["K0"],
                     c["state_idx"], c["flags"], c["H"], c["D"], mult=_mult(c, keep), drop=drop)
    rep = -(-c["N"] // r)
    t = (lambda x: np.tile(x, (rep,) + (1,) * (x.ndim - 1))[:c["N"]])
    return t(st["expect"]), st["stats"], t(keep), t(st["nz_cnt"])


# ----------------------------------------------------------------------------------------------------- pm_dsc_estep_f64
def _run_estep(dev, det, c, ref, layout, what):
    lib = _lib_of(det)
    H, Hp, S, N, Kt = c["H"], c["Hp"], c["S"], c["N"], c["Kt"]
    ops = _inputs(dev, c, layout)
    el = Emb(np.zeros((N, Kt)), _ld(Kt, layout, 1), dev, fill=False)
    es = Emb(np.zeros(N), N, dev, fill=False)
    P = _params(c)
    rc = lib.pm_dsc_estep_f64(ops["A"].ptr, ops["A"].ld, ops["G"].ptr, ops["yn"].ptr, ops["cand"].ptr, _tabptr(ops), S,
                              ops["prior"].ptr, ctypes.byref(P), N, H, Hp, el.ptr, el.ld, es.ptr, _stream())
    torch.cuda.synchronize()
    assert rc == 0, (what, rc)
    got, lse = el.host(), es.host()[0]
    assert np.array_equal(got, ref["F64"]), (what, "logpj", np.argwhere(got != ref["F64"])[:5].tolist())
    err = np.abs(lse.astype(LD) - ref["lse"])
    assert (err <= R.lse_bound(Kt, ref["lse"].astype(np.float64))).all(), (what, "lse", float(err.max()))
    assert el.outside_untouched() and es.outside_untouched() and _unchanged(ops), what
    return got, lse


# ---------------------------------------------------------------------------------------------- pm_dsc_estep_mstats_f64
def _run_mstats(dev, det, c, ref, layout, widen, lists, what):
    lib = _lib_of(det)
    H, Hp, S, N, D, Kt = c["H"], c["Hp"], c["S"], c["N"], c["D"], c["Kt"]
    ops = _inputs(dev, c, layout)
    el = Emb(np.zeros((N, Kt)), _ld(Kt, layout, 1), dev, fill=False)
    es = Emb(np.zeros(N), N, dev, fill=False)
    ee = Emb(np.zeros((N, H)), _ld(H, layout, 2), dev, fill=False)
    start = _stats_start(H, D)
    est = Emb(start, len(start), dev)
    ei = Emb(np.zeros((N, R.NZ_MAX), dtype=np.uint16), R.NZ_MAX, dev, fill=False)
    ev = Emb(np.zeros((N, R.NZ_MAX)), R.NZ_MAX, dev, fill=False)
    P = _params(c)
    rc = lib.pm_dsc_estep_mstats_f64(ops["A"].ptr, ops["A"].ld, ops["G"].ptr, ops["yn"].ptr, ops["cand"].ptr, _tabptr(ops), S,
                                     ops["prior"].ptr, ctypes.byref(P), N, H, D, Hp, el.ptr, el.ld, es.ptr, ee.ptr, ee.ld,
                                     est.ptr, ei.ptr if lists else None, ev.ptr if lists else None, _stream())
    torch.cuda.synchronize()
    if R.CASES[c["name"]][9 + R.MSTATS] is None:
        assert rc == PM_ERANGE and all(e.unchanged() for e in (el, es, ee, est, ei, ev)), (what, rc)
        return
    assert rc == 0, (what, rc)
    got, lse, exp, stats = el.host(), es.host()[0], ee.host(), est.host()[0]
    assert np.array_equal(got, ref["F64"]), (what, "logpj", np.argwhere(got != ref["F64"])[:5].tolist())
    err = np.abs(lse.astype(LD) - ref["lse"])
    assert (err <= R.lse_bound(Kt, ref["lse"].astype(np.float64))).all(), (what, "lse", float(err.max()))
    want_e, want_s, keep, nzc = _ref_rows(c, ref, ref["lse"], -np.inf, onepass=True)
    assert row_rel(exp.astype(LD), want_e) <= RTOL, (what, "expect", row_rel(exp.astype(LD), want_e))
    # (the reference's overflow count rests on exact zeros of E[s]; the lists are checked against the returned rows below)
    want_s = want_s.copy()
    want_s[-1] = 0
    if lists:
        counts = _check_lists(ei.host_u16(), ev, exp, keep, stats[-1], start[-1], what)
        want_s[-1] = int((counts > R.NZ_MAX).sum())
        if c["hot"] and c["K"] == 2 and not c["flags"]:
            assert np.array_equal(counts, nzc) and (counts == H).all(), (what, "non-zero counts")
    else:
        assert ei.unchanged() and ev.unchanged(), what
    _check_stats(stats, start, want_s, H, D, N, widen, what)
    assert all(e.outside_untouched() for e in (el, es, ee, est, ei, ev)) and _unchanged(ops), what


# ------------------------------------------------------------------------------- pm_dsc_mstep_rows_f64 / _nz / _cutp
def _run_rows(dev, det, c, ref, layout, widen, entry, lse_in, cut, what):
    """entry: "rows" (cut by value, no lists), "nz" (by value, lists), "cutp" (cut on the device, +inf by value; lists on
    the sixteen-lane family)."""
    lib = _lib_of(det)
    H, Hp, S, N, D, Kt = c["H"], c["Hp"], c["S"], c["N"], c["D"], c["Kt"]
    l16 = R.CASES[c["name"]][9 + R.ROWS][0] == R.L16
    ops = _inputs(dev, c, layout)
    del ops["A"], ops["G"], ops["yn"]
    ops["F"] = Emb(ref["F64"], _ld(Kt, layout, 1), dev)
    ops["lse"] = Emb(lse_in, N, dev)
    ops["cut"] = Emb(np.array([cut]), 1, dev)
    ee = Emb(np.zeros((N, H)), _ld(H, layout, 2), dev, fill=False)
    start = _stats_start(H, D)
    est = Emb(start, len(start), dev)
    ei = Emb(np.zeros((N, R.NZ_MAX), dtype=np.uint16), R.NZ_MAX, dev, fill=False)
    ev = Emb(np.zeros((N, R.NZ_MAX)), R.NZ_MAX, dev, fill=False)
    P = _params(c)
    head = (ops["F"].ptr, ops["F"].ld, ops["lse"].ptr)
    tail = (ops["cand"].ptr, _tabptr(ops), S, ops["prior"].ptr, ctypes.byref(P), N, H, D, Hp, ee.ptr, ee.ld, est.ptr)
    lists = entry == "nz" or (entry == "cutp" and l16)
    if entry == "rows":
        rc = lib.pm_dsc_mstep_rows_f64(*head, ctypes.c_double(cut), *tail, _stream())
    elif entry == "nz":
        rc = lib.pm_dsc_mstep_rows_nz_f64(*head, ctypes.c_double(cut), *tail, ei.ptr, ev.ptr, _stream())
    else:
        rc = lib.pm_dsc_mstep_rows_cutp_f64(*head, ctypes.c_double(np.inf), ops["cut"].ptr, *tail, ei.ptr if lists else None,
                                            ev.ptr if lists else None, _stream())
    torch.cuda.synchronize()
    if lists and not l16:         # lists come from the sixteen-lane kernel only
        assert rc == PM_ERANGE and all(e.unchanged() for e in (ee, est, ei, ev)), (what, rc)
        return None
    assert rc == 0, (what, rc)
    exp, stats = ee.host(), est.host()[0]
    want_e, want_s, keep, nzc = _ref_rows(c, ref, lse_in, cut)
    assert np.array_equal(exp[~keep], np.zeros((int((~keep).sum()), H))), (what, "cut rows are not zero")
    assert row_rel(exp.astype(LD), want_e) <= RTOL, (what, "expect", row_rel(exp.astype(LD), want_e))
    want_s = want_s.copy()
    want_s[-1] = 0
    if lists:
        counts = _check_lists(ei.host_u16(), ev, exp, keep, stats[-1], start[-1], what)
        want_s[-1] = int((counts[keep] > R.NZ_MAX).sum())
        if c["hot"] and c["K"] == 2 and not c["flags"]:
            assert np.array_equal(counts, nzc) and (counts[keep] == H).all(), (what, "non-zero counts")
    else:
        assert ei.unchanged() and ev.unchanged(), what
    _check_stats(stats, start, want_s, H, D, N, widen, what)
    assert all(e.outside_untouched() for e in (ee, est, ei, ev)) and _unchanged(ops), what
    return exp


def _cut_inputs(c, ref):
    """lse as the row pass receives it, with a NaN row (N >= 4), and a cut that EQUALS the lse of one datapoint bit for bit
    and lies above a third of the others."""
    lse = ref["lse"].astype(np.float64).copy()
    r = c["rows"]
    t = int(np.argsort(lse[:r], kind="stable")[r // 3])
    cut = float(lse[t])
    if r >= 4:
        lse[(t + 1) % r::r] = np.nan
    return lse, cut, t


@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_dispatch_cell(dev, name, det):
    """One dispatch cell (dsc_kernels_reference.CASES), hot and cold: the plan is the cell's; pm_dsc_estep_f64 and
    pm_dsc_estep_mstats_f64 (lists on when hot, off when cold) from the scores; the row pass from the exact log-joints
    through its three entry names -- cut by value at a datapoint whose lse equals the cut (strict: dropped, not counted),
    a NaN lse (dropped), lists on and off, the cut read from the device while the by-value cut is +inf."""
    i = CASE_NAMES.index(name)
    for hot in (True, False):
        c, ref = _case(name, hot)
        for which in (R.ESTEP, R.MSTATS, R.ROWS):
            rc, out = _plan(det, which, c)
            want = R.CASES[name][9 + which]
            assert (rc == PM_ERANGE) if want is None else (rc == 0 and out[:6] == want), (name, which, rc, out)
        layout = LAYOUTS[1 + (i + 2 * hot) % 4]
        widen = 0.0
        if det:
            widen = (c["N"] + 1) * _install_quanta(c, ref) / 2
        try:
            what = (name, "hot" if hot else "cold", "det" if det else "default", layout)
            _run_estep(dev, det, c, ref, layout, what + ("estep",))
            _run_mstats(dev, det, c, ref, layout, widen, hot, what + ("mstats",))
            lse_in, cut, t = _cut_inputs(c, ref)
            exp = _run_rows(dev, det, c, ref, layout, widen, "rows", lse_in, cut, what + ("rows",))
            assert not exp[t].any() and (c["rows"] < 4 or not exp[(t + 1) % c["rows"]].any()), what
            _run_rows(dev, det, c, ref, layout, widen, "nz", ref["lse"].astype(np.float64), -np.inf, what + ("rows_nz",))
            _run_rows(dev, det, c, ref, layout, widen, "cutp", lse_in, cut, what + ("rows_cutp",))
        finally:
            if det:
                from prosper_amd.em.camodels import _device
                _device._DET_QUANTA_SET.pop("dsc", None)


# ------------------------------------------------------------------------------------------------------ row independence
@pytest.mark.parametrize("name", ["l16_8_8", "l16_16_16", "wave8_h257", "wave16_lds_m", "tsc_l16"])
def test_rows_are_independent(dev, name):
    """A row permutation of the inputs permutes the logpj, lse and E[s] rows bit for bit (cold: weights of every size)."""
    c, ref = _case(name, False)
    N = c["N"]
    perm = np.random.RandomState(N).permutation(N)
    cp = dict(c, A=c["A"][perm], yn=c["yn"][perm], cand=c["cand"][perm])
    refp = dict(ref, E=ref["E"][perm], F=ref["F"][perm], F64=ref["F64"][perm], lse=ref["lse"][perm])
    what = (name, "permuted")
    F0, l0 = _run_estep(dev, False, c, ref, "odd", what)
    F1, l1 = _run_estep(dev, False, cp, refp, "odd", what)
    assert np.array_equal(F1, F0[perm]) and np.array_equal(l1.view(np.int64), l0[perm].view(np.int64)), what
    cut = float(np.sort(l0)[N // 3])
    # the periodic bookkeeping of _ref_rows does not apply to permuted rows: these cases have N = rows, mult = 1
    assert c["rows"] == N
    e0 = _run_rows(dev, False, c, ref, "even", 0.0, "rows", l0, cut, what)
    e1 = _run_rows(dev, False, cp, refp, "even", 0.0, "rows", l1, cut, what)
    assert np.array_equal(e1.view(np.int64), e0[perm].view(np.int64)), what


# --------------------------------------------------------------------------------------------------------- return codes
def test_return_codes_leave_the_outputs_untouched(dev):
    """Every PM_EINVAL / PM_ERANGE condition the three entry points state; nothing is launched (no output element moves)."""
    lib = _lib_of(False)
    c, ref = _case("l16_8_8", True)
    cw, refw = _case("wave8_h257", True)

    def call(entry, c, ref, **ov):
        H, Hp, S, N, D, Kt = c["H"], c["Hp"], c["S"], c["N"], c["D"], c["Kt"]
        ops = _inputs(dev, c, "odd")
        ops["F"], ops["lse"] = Emb(ref["F64"], Kt + 1, dev), Emb(ref["lse"].astype(np.float64), N, dev)
        outs = dict(el=Emb(np.zeros((N, Kt)), Kt + 1, dev, fill=False), es=Emb(np.zeros(N), N, dev, fill=False),
                    ee=Emb(np.zeros((N, H)), H + 1, dev, fill=False), est=Emb(_stats_start(H, D), R.stats_len(H, D), dev),
                    ei=Emb(np.zeros((N, 16), dtype=np.uint16), 16, dev, fill=False), ev=Emb(np.zeros((N, 16)), 16, dev, fill=False))
        P = _params(c, **{k: v for k, v in ov.items() if k in ("K", "K0", "ecoef")})
        if "v0" in ov:
            P.values[c["K0"]] = ov["v0"]
        g = lambda k, d: ov.get(k, d)
        nzi, nzv = g("nzi", outs["ei"].ptr), g("nzv", outs["ev"].ptr)
        Hp, H2, D = g("Hp", Hp), g("H", H), g("D", D)
        tab = g("tab", _tabptr(ops))
        if entry == "estep":
            rc = lib.pm_dsc_estep_f64(g("A", ops["A"].ptr), g("lds", ops["A"].ld), ops["G"].ptr, ops["yn"].ptr, ops["cand"].ptr,
                                      tab, S, ops["prior"].ptr, ctypes.byref(P), g("N", N), H2, Hp, outs["el"].ptr,
                                      g("ldl", Kt + 1), outs["es"].ptr, _stream())
        elif entry == "mstats":
            rc = lib.pm_dsc_estep_mstats_f64(g("A", ops["A"].ptr), g("lds", ops["A"].ld), ops["G"].ptr, ops["yn"].ptr,
                                             ops["cand"].ptr, tab, S, ops["prior"].ptr, ctypes.byref(P), g("N", N), H2, D, Hp,
                                             outs["el"].ptr, g("ldl", Kt + 1), outs["es"].ptr, outs["ee"].ptr, g("lde", H + 1),
                                             outs["est"].ptr, nzi, nzv, _stream())
        else:
            rc = lib.pm_dsc_mstep_rows_cutp_f64(g("F", ops["F"].ptr), g("ldl", Kt + 1), ops["lse"].ptr, ctypes.c_double(-np.inf),
                                                None, ops["cand"].ptr, tab, S, ops["prior"].ptr, ctypes.byref(P), g("N", N), H2,
                                                D, Hp, outs["ee"].ptr, g("lde", H + 1), outs["est"].ptr, nzi, nzv, _stream())
        torch.cuda.synchronize()
        assert all(e.unchanged() for e in outs.values()) and _unchanged(ops), (entry, ov)
        return rc

    Kt, H = c["Kt"], c["H"]
    for entry in ("estep", "mstats", "rows"):
        assert call(entry, c, ref, ldl=Kt - 1) == PM_EINVAL, entry
        assert call(entry, c, ref, K=9) == PM_EINVAL and call(entry, c, ref, K=1) == PM_EINVAL, entry
        assert call(entry, c, ref, K0=c["K"]) == PM_EINVAL and call(entry, c, ref, v0=1.0) == PM_EINVAL, entry
        assert call(entry, c, ref, tab=None) == PM_EINVAL, entry                        # S > 0 without a state table
        assert call(entry, c, ref, N=-1) == PM_EINVAL and call(entry, c, ref, Hp=0) == PM_EINVAL, entry
        assert call(entry, c, ref, Hp=17) == PM_ERANGE, entry                           # > PM_MAX_HPRIME (H = 17)
        assert call(entry, c, ref, Hp=4, H=3, ldl=10 ** 6) == PM_ERANGE, entry           # H' > H
        assert call(entry, c, ref, N=0, nzi=None) == (PM_OK if entry == "estep" else PM_EINVAL), entry
    for entry in ("estep", "mstats"):
        assert call(entry, c, ref, lds=H - 1) == PM_EINVAL and call(entry, c, ref, A=None) == PM_EINVAL, entry
    for entry in ("mstats", "rows"):
        assert call(entry, c, ref, ecoef=0.0) == PM_EINVAL and call(entry, c, ref, lde=H - 1) == PM_EINVAL, entry
        assert call(entry, c, ref, nzi=None) == PM_EINVAL and call(entry, c, ref, nzv=None) == PM_EINVAL, entry
        assert call(entry, c, ref, D=0) == PM_EINVAL, entry
    assert call("rows", c, ref, F=None) == PM_EINVAL
    # wave-path shapes: no one-pass statistics, no lists
    assert call("mstats", cw, refw) == PM_ERANGE and call("mstats", cw, refw, nzi=None, nzv=None) == PM_ERANGE
    assert call("rows", cw, refw) == PM_ERANGE



# ------------------------------------------------------------------------------------------------------------ selection
SEL_VALUES, SEL_K0 = np.array([2.0, 0.0, -1.0, 3.0]), 1
SEL_LOGPI = np.array([-1.25, -0.5, -2.0, -0.75])
SEL_PRE1 = -0.125


def _sel_operands(N, H, seed):
    """Integer scores; a Gram matrix whose off-diagonal is junk no selection may read (the diagonal is |W_h|^2)."""
    A = R.ints(N, H, seed)
    G = 1000.0 + R.ints(H, H, seed + 1, 0, 50)
    G[np.arange(H), np.arange(H)] = 1.0 + (np.arange(H) * 5 + seed) % 9
    return A, G


def _sel_params():
    c = dict(K=4, K0=SEL_K0, values=SEL_VALUES, ecoef=-1.0, pscale=1.0, flags=0)
    P = _params(c, pre1=SEL_PRE1)
    for k in range(4):
        P.logpi[k] = SEL_LOGPI[k]
    return P


@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
@pytest.mark.parametrize("H", [1, 17, 256, 300])
def test_select_scores(dev, H, det):
    """pm_dsc_select_scores_f64 and pm_tsc_select_scores_f64 equal the reference (every product and sum is exact), padded
    lds / ldr, N of 1 and 70."""
    lib = _lib_of(det)
    for N in (1, 70):
        A, G = _sel_operands(N, H, N + H)
        for k, layout in enumerate(LAYOUTS):
            eA, eG = Emb(A, _ld(H, layout, 0), dev), Emb(G, H, dev)
            want = R.dsc_select_scores(A, G, SEL_VALUES, SEL_K0, SEL_LOGPI, SEL_PRE1)
            eR = Emb(np.zeros((N, H)), _ld(H, layout, 1), dev, fill=False)
            P = _sel_params()
            assert lib.pm_dsc_select_scores_f64(eA.ptr, eA.ld, eG.ptr, ctypes.byref(P), N, H, eR.ptr, eR.ld, _stream()) == 0
            torch.cuda.synchronize()
            assert np.array_equal(eR.host().astype(LD), want), (N, H, layout, "dsc")
            assert eR.outside_untouched() and eA.unchanged() and eG.unchanged(), (N, H, layout)
            want = R.tsc_select_scores(A, G)
            eR = Emb(np.zeros((N, 2 * H)), _ld(2 * H, layout, 1), dev, fill=False)
            assert lib.pm_tsc_select_scores_f64(eA.ptr, eA.ld, eG.ptr, N, H, eR.ptr, eR.ld, _stream()) == 0
            torch.cuda.synchronize()
            assert np.array_equal(eR.host().astype(LD), want), (N, H, layout, "tsc")
            assert eR.outside_untouched() and eA.unchanged() and eG.unchanged(), (N, H, layout)
    # what a wrong tie rule or value index would hide behind: the best value differs between latents
    A, G = _sel_operands(70, max(H, 2), 5)
    best = np.stack([SEL_PRE1 * (v * v * np.diag(G)[None, :] - 2 * v * A) + lp
                     for v, lp in zip(SEL_VALUES[[0, 2, 3]], SEL_LOGPI[[0, 2, 3]])]).argmax(axis=0)
    assert H == 1 or len(np.unique(best)) >= 2


@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
@pytest.mark.parametrize("tsc,H", [(0, 3), (0, 16), (0, 17), (0, 128), (0, 129), (0, 256),
                                   (1, 16), (1, 32), (1, 64), (1, 128), (1, 256)])
def test_fused_selection_against_the_reference_ranking(dev, tsc, H, det):
    """pm_xsc_select_f64 equals the reference's stable ranking of the reference's scores -- never the library's two-launch
    form: integer scores make the ties real (DSC: the smaller latent first; TSC: ascending, of equal one-cause states the
    larger index last, then state % H).  N of 1 and 70 (not a multiple of the 16-row groups), H' of 1, 8 and 16."""
    lib = _lib_of(det)
    ties = 0
    for N in (1, 70):
        A, G = _sel_operands(N, H, 3 * N + H + tsc)
        for Hp in (1, 8, 16):
            if Hp > H:
                continue
            assert lib.pm_xsc_select_supported(H, Hp, tsc)
            eA, eG = Emb(A, _ld(H, LAYOUTS[1 + Hp % 4], 0), dev), Emb(G, H, dev)
            if tsc:
                Rm = R.tsc_select_scores(A, G)
                want = R.rank_largest_best_last(Rm, Hp) % H
                srt = np.sort(Rm, axis=1)[:, ::-1]
            else:
                Rm = R.dsc_select_scores(A, G, SEL_VALUES, SEL_K0, SEL_LOGPI, SEL_PRE1)
                want = R.rank_smallest_first(Rm, Hp)
                srt = np.sort(Rm, axis=1)
            if Hp < Rm.shape[1]:
                ties += int((srt[:, Hp - 1] == srt[:, Hp]).sum())          # a tie across the selection boundary
            ec = _odd(np.zeros((N, Hp), dtype=np.int32), Hp, dev, fill=False)
            P = _sel_params()
            rc = lib.pm_xsc_select_f64(eA.ptr, eA.ld, eG.ptr, None if tsc else ctypes.byref(P), N, H, Hp, ec.ptr, _stream())
            torch.cuda.synchronize()
            assert rc == 0, (tsc, H, Hp, N, rc)
            got = ec.host()
            assert np.array_equal(got, want), (tsc, H, Hp, N, np.argwhere(got != want)[:5].tolist())
            assert ec.outside_untouched() and eA.unchanged() and eG.unchanged(), (tsc, H, Hp, N)
    assert H < 64 or ties > 0, (tsc, H, "no tie across the selection boundary in these data")


@pytest.mark.parametrize("tsc,H,Hp", [(0, 1024, 8), (1, 17, 8), (1, 512, 4), (0, 16, 17)])
def test_fused_selection_unsupported_shapes(dev, tsc, H, Hp):
    """PM_ERANGE, and not an element of the candidates is written."""
    lib = _lib_of(False)
    assert not lib.pm_xsc_select_supported(H, Hp, tsc)
    N = 5
    A, G = _sel_operands(N, H, H)
    eA, eG = Emb(A, H, dev), Emb(G, H, dev)
    ec = Emb(np.zeros((N, Hp), dtype=np.int32), Hp, dev, fill=False)
    P = _sel_params()
    rc = lib.pm_xsc_select_f64(eA.ptr, eA.ld, eG.ptr, None if tsc else ctypes.byref(P), N, H, Hp, ec.ptr, _stream())
    torch.cuda.synchronize()
    assert rc == PM_ERANGE and ec.unchanged()
