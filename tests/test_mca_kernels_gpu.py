"""The MCA / MMCA kernels (mca_kernels.hip) through the C ABI -- pm_mca_select_scores_f64, pm_mca_estep_f64,
pm_mca_mstep_rows_f64, pm_mca_estep_mstats_f64, pm_mca_estep_mstats_defer_f64 + pm_mca_defer_apply_f64, pm_mca_w_update_f64 -- on
padded, guarded operands, one smallest shape per dispatch cell (confirmed with pm_mca_plan inside the test: a case that lands
in another instantiation fails), against the plain NumPy reference tests/mca_kernels_reference.py, from both libraries.

Harness: ``Emb`` of tests/test_eval_kernels_gpu.py (16 guard rows before and after, padding columns, a quiet-NaN payload /
0xDEADBEEF pattern; 0xA5A5 for the uint16 state masks, carried as int16).  `cand` and `state_masks` start at odd element
offsets; scores, Y, the log-joints and q1 have padded leading dimensions.  After every call the result block is compared with
the reference, every guard and padding element of every output still holds the pattern, every input is bit-unchanged, and the
scratch tail of `stats` (the 7 * 2 H D per-XCD copies) is all zeros again.  `stats` starts from position-dependent multiples
of 1/8, so that "accumulates into" is tested; entries no datapoint contributes to come back bit-unchanged.

Exact (equality): the selection scores on integers (sum max(W, y) - sum y is exact in any order), pm_mca_defer_apply_f64 on
integer records, scalars, q1, Y and log-denominators with ties at the cut (every sum an exact integer in any order; the
deterministic library with a quantum of 2^-11, of which every integer is a multiple), pm_mca_w_update_f64 on integer
statistics and powers of two in W (G1 W^2 + Wp_m is exact with or without a fused multiply-add, the division is correctly
rounded on both sides).

Bounded: log-joints, lse1, lseb, q1, the deferred records and the statistics use the 1e-11 row-relative bound of
tests/test_eval_kernels_gpu.py (RTOL) against the longdouble reference: log-joints relative to the row's largest |f|, the
log-evidences relative to max(|lse|, the row's largest |f|), q1 and a datapoint's record block relative to their largest
entry, a statistic relative to the largest |value| of its section ([Wp_m], [Wq_m], [q1sum], each scalar on its own).  Values in
the subnormal range carry no relative precision: 1e-290 is added to every bound.  Such bounds cannot see a dropped state of
weight 1e-12, so every case runs HOT (pre1 = -2^-24, flat prior: all weights of a row within a factor e, a dropped, doubled
or misplaced state moves a result by ~1 / (1 + H + S)) and COLD (states on both sides of the -745 / -745.2 / underflow
cut-offs; tests/test_mca_kernels_cpu.py asserts both properties for every case).

Deterministic library: quanta for unit `mca` are installed as det_quanta of tests/test_dense_kernels_gpu.py does for `gemm`.
With A >= every |addend| and every |partial sum| of a section -- A = 4 (max |start + result| + N (1 + max |y|) max(1, max Aid))
-- the bound is 2^k >= A and the quantum 2^(k - 51).  A statistic receives at most N quantised addends per launch (one per
datapoint and element for Wp_m / Wq_m / q1sum, one per workgroup for the scalars), each off by at most quantum / 2, and the
fold of the per-XCD copies is exact on multiples of the quantum: the bound widens by (N + 1) quantum / 2.

The rescaling branch of the fused pass (`bf > M + 50`): cases `resc_*` put a prior of pil_bar = 64 T on a flat likelihood, so
beta f_s = 64 |s| + O(1e-5) and the order of the state table alone decides at which state the reference level moves (asserted
on the CPU by emulating the lazy maximum): at state 1, in the middle, at the last state, and on a paired tile at both states
of a trip and at the second only.  The states before a move weigh e^-64 of the result, so these cases see a rescaling that is
missing, doubled or applied with the wrong factor, not its last bits.

The sum q e (sigma) statistic and the deferred sigma scalar.  The kernels recover a state's energy from its log-joint, e_k =
(f_k - pil_bar |s_k|) / pre1 (the two-pass M-step for the singletons too), which cancels where |pre1 e_k| << |pil_bar| |s_k|: f_k
carries up to 2 u |f_k| from its own rounding and the product u |pil_bar| |s_k|, so e_k is off by up to u (2 |f_k| + |pil_bar|
|s_k|) / |pre1| whatever its size, and sum_k q_k e_k by u sum_k q_k (2 |f_k| + |pil_bar| |s_k|) / |pre1|
(mca_kernels_reference.sigma_cancellation).  That term, with the factor 4 of tests/test_dsc_kernels_gpu.py, is added to the
bound of the sigma scalar of a record and, summed over the kept datapoints, to that of the sigma statistic -- nowhere else.
In the ordinary cases it is below 1e-12 of the value; in the `resc_*` cases (|f| = 250, pre1 = -2^-24) it is 3.7e-6 per
datapoint; measured there: 3.6e-6 in the statistic (16 datapoints), 4.4e-7 in a record's scalar.

Element-wise: test_mstep_rows_elementwise compares Wp_m / Wq_m of the two-pass M-step element by element where an element
is dominated by a state of vanishing posterior (bound derived in its docstring), test_fused_elementwise does so for the fused pass in-pass and deferred + apply, from
data.

Mutants of mca_kernels.hip (values and predicates only), each run once against this module, default library, MI355X
(215 tests pass on the unchanged source):
  `lb >= lse_cut` -> `>` (M-step)                  50 fail: test_mstep_rows at every case, "tie" (the datapoint at the cut)
  `lseb[n] >= cut` -> `>` (scatter kernel only)    45: test_defer_apply_exact at all 9 shapes (cut 0 and 1 are ties),
                                                   test_fused_deferred at all 36 cases, "tie"
  `qcut` -745.2 -> -30                             1: test_mstep_rows_elementwise (no section-relative bound sees it)
  `sc = exp(M - bf)` -> 1.0                        67: test_fused_rescale at all 7 cases, test_fused and test_fused_deferred at
                                                   30 cases each (COLD: the reference level moves after the first state)
  `first` always true                              8: test_mstep_rows at the multi-slab cases u_d513, u_d1024, u_hp9, u_hp9_513,
                                                   u_hp13, u_hp13_257, u_hp4_513, s_hp16
  the `for (; g < G; ++g)` tail dropped            51: test_defer_apply_exact at the 7 shapes with G of 1, 2, 5 (G = 64 passes),
                                                   test_fused_deferred (36), test_fused_rescale (7) and the deferred
                                                   test_fused_elementwise, all G = 1
  `copysign` dropped in the E-step's signed Wbar   25: test_estep at every s_* case
  `hp <= 8 ? 8` -> `hp <= 9 ? 8` (fused tile)      the plan assertions of u_d128_12, s_p12_2b, s_p12_4 (_assert_cell, before any
                                                   launch; the same three in tests/test_mca_kernels_cpu.py::test_case_cells)
  `pfx = 0xFFFFFFFFu` reset after staging removed  0: equivalent -- `Pf` / `pfx` of mca_mstep_rows_kernel are declared inside the
                                                   datapoint loop and T_of is never called before the rows are staged
  signed padding `s_wm` 1.0 -> 0.0                 0: equivalent -- padding rows j >= H' are in no state mask; padding columns
                                                   d >= D hold T = 0, where fmin(w, w * inf * wm) is w for wm = 1 (inf) and for
                                                   wm = 0 (NaN), and are never stored
"""
import ctypes
import functools

import numpy as np
import pytest

import mca_kernels_reference as R
from test_eval_kernels_gpu import GUARD_ROWS, LAYOUTS, RTOL, Emb as _Emb, _ld, _stream, dev, ints, row_rel  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT_U16 = 0xA5A5 - 0x10000
PM_OK, PM_EINVAL, PM_ERANGE = 0, -1, -2
LD = np.longdouble
FLOOR = 1e-290
CASE_NAMES = list(R.CASES)
FUSED_NAMES = [n for n in CASE_NAMES if R.CASES[n][8][R.FUSED] is not None]
ALL_LAYOUT_CASE = "u_d65"           # the cell of every entry point that runs in all five layouts
WORST = {}                          # (entry, quantity, hot) -> largest error / bound seen (_report_worst_errors prints it)


class Emb(_Emb):
    """... and the uint16 state masks, carried as int16."""
    _TYPES = dict(_Emb._TYPES)
    _TYPES[np.dtype(np.int16)] = (torch.int16, SENT_U16)


def _odd(array, ld, dev):
    """An operand that starts at an odd element offset of its buffer."""
    e = Emb(array, ld, dev, off=1 if (GUARD_ROWS * ld) % 2 == 0 else 2)
    assert e.start % 2 == 1
    return e


def _lib_of(det):
    from prosper_amd import _lib
    return _lib.load(det)


def _params(c):
    from prosper_amd import _lib
    P = _lib.McaParams()
    P.pil_bar, P.pre1, P.beta, P.inv_rho, P.signed_w = c["pil_bar"], c["pre1"], c["beta"], c["inv_rho"], float(c["signed"])
    return P


def _plan(det, which, c, defer=0, **over):
    d = dict(H=c["H"], D=c["D"], Hp=c["Hp"], S=c["S"], N=c["N"])
    d.update(over)
    out = (ctypes.c_int32 * R.PLAN_LEN)(*([-7] * R.PLAN_LEN))
    rc = _lib_of(det).pm_mca_plan(which, d["H"], d["D"], d["Hp"], d["S"], int(c["signed"]), c["inv_rho"], d["N"], defer, out)
    return rc, tuple(out)


def _assert_cell(det, which, c, defer=0):
    """The case lands in the instantiation it is meant for; returns the plan."""
    want = c["cells"][which]
    rc, p = _plan(det, which, c, defer)
    if want is None:
        assert rc == PM_ERANGE, (c["name"], which, rc)
        return None
    got = p[:4] + (p[7:10] if which == R.MSTEP_ROWS else ())
    assert rc == PM_OK and got == want, (c["name"], which, rc, p)
    if c["N"] > 8192:
        assert p[6] == 2048, ("the grid is the cap", p)
    return p


@functools.lru_cache(maxsize=None)
def _case(name, hot):
    """Operands and reference of a case, computed once and shared by every test (and both libraries)."""
    c = R.make_case(name, hot) if name in R.CASES else R.make_rescale_case(name)
    return c, R.case_reference(c)


@functools.lru_cache(maxsize=None)
def _fused_ref(name, hot):
    """Statistics of the one-pass form with every datapoint kept, the deferred records and scalars (distinct rows)."""
    c, ref = _case(name, hot)
    r = slice(0, c["rows"])
    add, q1, aid = R.packed_stats(c, ref["F"], ref["lse1"], ref["lseb"], np.ones(c["rows"], dtype=bool), mult=R.mult(c), rows=r)
    rec, sc = R.defer_records(c, ref["F"], ref["lse1"], ref["lseb"], rows=r)
    canc = R.sigma_cancellation(c, ref["F"], R.posteriors(c, ref["F"], ref["lseb"]), singles=False)
    return add, q1, rec, sc, canc


def _inputs(dev, c, layout):
    H, D, Hp, S, N = c["H"], c["D"], c["Hp"], c["S"], c["N"]
    ops = dict(scores=Emb(c["scores"], _ld(H, layout, 0), dev), wn=Emb(c["wnorm2"], H, dev), yn=Emb(c["ynorm2"], N, dev),
               Y=Emb(c["Y"], _ld(D, layout, 1), dev), Wrho=Emb(c["Wrho"], D, dev), Wrm1=Emb(c["Wrm1"], D, dev),
               cand=_odd(c["cand"], Hp, dev))
    ops["masks"] = _odd(c["masks"].view(np.int16), S, dev) if S else None
    return ops


def _mptr(ops):
    return ops["masks"].ptr if ops["masks"] is not None else None


def _unchanged(ops):
    return all(e.unchanged() for e in ops.values() if e is not None)


def _stats_start(H, D, det):
    """Non-zero, position-dependent multiples of 1/8 in the documented part; the scratch tail starts (and must end) at zero."""
    n = int(_lib_of(det).pm_mca_stats_len(H, D))
    s = np.zeros(n)
    base = R.stats_base(H, D)
    s[:base] = (1 + (np.arange(base) * 5) % 8) / 8.0
    return s


def _install_quanta(c, total, aid_max):
    """Quanta of unit `mca` in the deterministic library (module docstring); returns the quantum."""
    from prosper_amd import _lib
    from prosper_amd.em.camodels import _device
    A = 4.0 * (float(np.abs(total).max()) + c["N"] * (1.0 + float(np.abs(c["Y"]).max())) * max(1.0, aid_max))
    k = int(np.ceil(np.log2(A)))
    M8 = (ctypes.c_double * 8)(*([1.5 * 2.0 ** (k + 1)] * 8))
    _device._DET_QUANTA_SET.pop("mca", None)
    _lib.call("pm_det_set_quanta", _lib.DET_UNITS["mca"], M8, _stream(), det=True)
    torch.cuda.synchronize()
    return 2.0 ** (k - 51)


def _note(entry, what, hot, err, bound):
    key = (entry, what, "HOT" if hot else "COLD")
    ratio = float(err) / float(bound) if bound > 0 else 0.0
    if ratio > WORST.get(key, (0.0, 0.0, 0.0))[0]:
        WORST[key] = (ratio, float(err), float(bound))


def _close_rows(got, want, scale_extra, entry, what, hot, tag, extra=0.0):
    """Row-relative: every row of got within RTOL of the row's largest |want| (or scale_extra, if larger)."""
    want = np.asarray(want, dtype=LD)
    got = np.asarray(got).astype(LD)
    if want.ndim == 1:
        want, got = want[:, None], got[:, None]
    scale = np.abs(want).max(axis=1)
    if scale_extra is not None:
        scale = np.maximum(scale, scale_extra)
    err = np.abs(got - want).max(axis=1)
    bound = RTOL * scale + FLOOR + extra
    i = int(np.argmax(err / bound))
    _note(entry, what, hot, err[i], bound[i])
    assert (err <= bound).all(), (tag, what, "row", i, float(err[i]), float(bound[i]))


def _check_stats(got, start, add, c, widen, entry, tag, exact_count=True, sigma_extra=0.0):
    H, D, hot = c["H"], c["D"], c["hot"]
    HD, base = H * D, R.stats_base(H, D)
    total = start[:base].astype(LD) + add
    assert np.array_equal(got[:HD], start[:HD]), (tag, "the G1 section was written")
    assert not got[base:].any(), (tag, "the scratch tail is not zero again")
    zero = np.asarray(add == 0)
    assert np.array_equal(got[:base][zero], start[:base][zero]), (tag, "an entry no datapoint contributes to was written",
                                                                  np.nonzero(got[:base][zero] != start[:base][zero])[0][:5])
    o = 3 * HD + H
    secs = dict(Wp=slice(HD, 2 * HD), Wq=slice(2 * HD, 3 * HD), q1sum=slice(3 * HD, o), pi=slice(o, o + 1),
                sigma=slice(o + 1, o + 2), lse=slice(o + 2, o + 3), count=slice(o + 3, o + 4))
    for sec, sl in secs.items():
        scale = float(np.abs(total[sl]).max())
        err = float(np.abs(got[sl].astype(LD) - total[sl]).max())
        bound = RTOL * scale + widen + FLOOR + (float(sigma_extra) if sec == "sigma" else 0.0)
        _note(entry, "stats." + sec, hot, err, bound)
        assert err <= bound, (tag, sec, err, bound)
    if exact_count and widen == 0.0:
        assert got[o + 3] == float(total[o + 3]), (tag, "count")


def _layouts(name):
    return LAYOUTS if name == ALL_LAYOUT_CASE else ["tight", "odd"]


# ------------------------------------------------------------------------------------------- pm_mca_select_scores_f64
@pytest.mark.parametrize("H", [1, 63, 64, 65, 70])
def test_select_scores_exact(dev, H):
    """R[n,h] = sum_d max(W_hd - y_d, 0) on integers, negative y and W included: equality.  64 x 64 output tiles over 16-wide
    slabs of D: every tile edge in N, H and D."""
    k = 0
    for N in (1, 63, 64, 65, 130):
        for D in (1, 15, 16, 17, 33):
            Y, W = ints(N, D, N + D), ints(H, D, H * D + 1)
            want = R.select_scores(Y, W).astype(np.float64)
            for det in (False, True) if D == 17 else (False,):
                layout = LAYOUTS[k % len(LAYOUTS)]
                k += 1
                ey, ew = Emb(Y, _ld(D, layout, 0), dev), Emb(W, _ld(D, layout, 1), dev)
                er = Emb(np.zeros((N, H)), _ld(H, layout, 2), dev, fill=False)
                rc = _lib_of(det).pm_mca_select_scores_f64(ey.ptr, ey.ld, ew.ptr, ew.ld, er.ptr, er.ld, N, H, D, _stream())
                torch.cuda.synchronize()
                tag = (N, H, D, layout, det)
                assert rc == 0 and np.array_equal(er.host(), want), tag
                assert er.outside_untouched() and ey.unchanged() and ew.unchanged(), tag


# ------------------------------------------------------------------------------------------------ pm_mca_w_update_f64
@pytest.mark.parametrize("shape", [(1, 1), (5, 51), (16, 16), (1, 257), (3, 6)])
def test_w_update_exact(dev, shape):
    """wt_new = (G1 W^2 + Wp_m) / (q1sum W^2 + Wq_m) on integer statistics and powers of two in W: equality.  Row 0 has q1sum = 0
    and denominators 0, negative, a subnormal, exactly the smallest normal, half of it, and ordinary values; wt_clamped given
    and NULL; H D of 1, 255, 256, 257."""
    H, D = shape
    HD = H * D
    special = [0.0, -3.0, 5e-324, R.TINY, R.TINY / 2, 2.0, 1e-310, 4.0]
    for which, det in ((k, d) for k in range(len(special) if HD == 1 else 1) for d in (False, True)):
        rng = np.random.RandomState(HD + which)
        W = rng.choice([0.5, 1.0, 2.0, 4.0], size=(H, D))
        stats = np.zeros(R.stats_base(H, D))
        stats[:2 * HD] = rng.randint(-8, 9, size=2 * HD)
        stats[2 * HD:3 * HD] = rng.randint(0, 9, size=HD)
        stats[3 * HD:3 * HD + H] = rng.randint(0, 5, size=H)
        stats[3 * HD] = 0.0
        stats[2 * HD:2 * HD + min(D, len(special))] = (special[which:] + special[:which])[:min(D, len(special))]
        stats[-4:] = [3.0, 5.0, -7.0, 9.0]
        want, want_c = R.w_update(stats, W, H, D, 0.25)
        for clamped in (True, False):
            es, ew = Emb(stats, len(stats), dev), Emb(W, D, dev)
            eo, ec = Emb(np.zeros((H, D)), D, dev, fill=False), Emb(np.zeros((H, D)), D, dev, fill=False)
            rc = _lib_of(det).pm_mca_w_update_f64(es.ptr, ew.ptr, H, D, ctypes.c_double(0.25), eo.ptr, ec.ptr if clamped else None,
                                                  _stream())
            torch.cuda.synchronize()
            tag = (shape, which, det, clamped)
            assert rc == 0 and np.array_equal(eo.host(), want), tag
            assert np.array_equal(ec.host(), want_c) if clamped else ec.unchanged(), tag
            assert eo.outside_untouched() and ec.outside_untouched() and es.unchanged() and ew.unchanged(), tag


# ---------------------------------------------------------------------------------------------- pm_mca_defer_apply_f64
APPLY_SHAPES = {          # name: (N, H, Hprime, D, (DPL, HR, latent ranges, groups))
    "d1": (1, 3, 1, 1, (1, 3, 1, 1)),
    "d64": (255, 5, 2, 64, (1, 5, 1, 1)),
    "d64_2ranges": (257, 129, 3, 64, (1, 128, 2, 2)),          # a last range of one latent
    "d65_2ranges": (1100, 65, 3, 65, (2, 64, 2, 5)),           # five groups: the tail loop of the reduce kernel
    "d129_2ranges": (300, 33, 12, 129, (4, 32, 2, 2)),
    "d257_2ranges": (257, 17, 2, 257, (8, 16, 2, 2)),
    "d512": (300, 20, 12, 512, (8, 16, 2, 2)),
    "g64": (16200, 7, 3, 64, (1, 7, 1, 64)),
    "trip2": (65600, 3, 2, 2, (1, 3, 1, 64)),                  # 65 datapoints per wavefront: its second trip of 64
}


@pytest.mark.parametrize("name", list(APPLY_SHAPES))
def test_defer_apply_exact(dev, name):
    """Integer records, scalars, q1, Y and log-denominators with ties at the cut: every sum is an exact integer in any order,
    so the statistics equal the reference over the kept set, the q1 rows of the dropped datapoints are zero and those of the
    kept ones untouched -- from both libraries; the shape d65_2ranges in all five LAYOUTS.  Datapoint 0 has all its candidates in the first latent range and none in a
    second one."""
    N, H, Hp, D, cell = APPLY_SHAPES[name]
    rng = np.random.RandomState(N + H + D)
    c = dict(H=H, D=D, Hp=Hp, S=0, N=N, signed=0, inv_rho=0.5)
    lseb = rng.randint(-3, 4, size=N).astype(np.float64)
    Y = rng.randint(-3, 4, size=(N, D)).astype(np.float64)
    cand = np.stack([rng.permutation(H)[:Hp] for _ in range(min(N, 97))]).astype(np.int32)
    cand = np.tile(cand, (-(-N // len(cand)), 1))[:N]
    cand[0] = np.arange(Hp)              # all in the first latent range, none in a second one
    assert cand[0].max() < cell[1]
    rec = rng.randint(-3, 4, size=(N, Hp * D)).astype(np.float64)
    sc = rng.randint(-5, 6, size=(N, 4)).astype(np.float64)
    q1 = rng.randint(0, 4, size=(N, H)).astype(np.float64)
    for det in (False, True):
        rc, p = _plan(det, R.DEFER_APPLY, c)
        assert rc == PM_OK and (p[0], p[11], p[12], p[13]) == cell, (name, p)
        if det:
            from prosper_amd import _lib
            from prosper_amd.em.camodels import _device
            M8 = (ctypes.c_double * 8)(*([1.5 * 2.0 ** 41] * 8))
            _device._DET_QUANTA_SET.pop("mca", None)
            _lib.call("pm_det_set_quanta", _lib.DET_UNITS["mca"], M8, _stream(), det=True)
        lib = _lib_of(det)
        wlen = int(lib.pm_mca_defer_apply_work_len(H, D))
        for cut, layout in [(-10.0, "odd"), (10.0, "odd"), (0.0, "tight"), (1.0, "odd")] + \
                ([(0.0, lay) for lay in LAYOUTS] if name == "d65_2ranges" else []):
            start = np.zeros(int(lib.pm_mca_stats_len(H, D)))
            base = R.stats_base(H, D)
            start[:base] = 1 + (np.arange(base) * 5) % 8
            ops = dict(lseb=Emb(lseb, N, dev), cut=Emb(np.array([cut]), 1, dev), Y=Emb(Y, _ld(D, layout, 0), dev),
                       cand=_odd(cand, Hp, dev), rec=Emb(rec, Hp * D, dev), sc=Emb(sc, 4, dev))
            eq, est = Emb(q1, _ld(H, layout, 1), dev), Emb(start, len(start), dev)
            ew = Emb(np.zeros(wlen), wlen, dev, fill=False)
            rc = lib.pm_mca_defer_apply_f64(ops["lseb"].ptr, ops["cut"].ptr, ops["Y"].ptr, ops["Y"].ld, ops["cand"].ptr,
                                            ops["rec"].ptr, ops["sc"].ptr, eq.ptr, eq.ld, est.ptr, ew.ptr, N, H, D, Hp, _stream())
            torch.cuda.synchronize()
            tag = (name, det, cut)
            assert rc == 0, tag
            add, q1_want, keep = R.defer_apply(H, D, lseb, cut, Y, cand, rec.reshape(N, Hp, D), sc, q1)
            assert keep.all() if cut == -10.0 else not keep.any() if cut == 10.0 else True
            got = est.host()[0]
            assert np.array_equal(got[:base], (start[:base] + add).astype(np.float64)), (tag, "statistics")
            assert not got[base:].any(), (tag, "the scratch tail")
            assert np.array_equal(eq.host(), q1_want), (tag, "q1")
            assert eq.outside_untouched() and est.outside_untouched() and ew.outside_untouched() and _unchanged(ops), tag
    from prosper_amd.em.camodels import _device
    _device._DET_QUANTA_SET.pop("mca", None)


# ----------------------------------------------------------------------------------------------------- pm_mca_estep_f64
def _run_estep(dev, det, c, ref, layout):
    H, D, Hp, S, N = c["H"], c["D"], c["Hp"], c["S"], c["N"]
    ops = _inputs(dev, c, layout)
    K = 1 + H + S
    el = Emb(np.zeros((N, K)), _ld(K, layout, 2), dev, fill=False)
    e1, eb = Emb(np.zeros(N), N, dev, fill=False), Emb(np.zeros(N), N, dev, fill=False)
    P = _params(c)
    rc = _lib_of(det).pm_mca_estep_f64(ops["scores"].ptr, ops["scores"].ld, ops["wn"].ptr, ops["yn"].ptr, ops["Y"].ptr,
                                       ops["Y"].ld, ops["Wrho"].ptr, ops["cand"].ptr, _mptr(ops), S, ctypes.byref(P), N, H, D, Hp,
                                       el.ptr, el.ld, e1.ptr, eb.ptr, _stream())
    torch.cuda.synchronize()
    tag = (c["name"], c["hot"], det, layout, "estep")
    assert rc == 0, tag
    _check_e(c, ref, el, e1, eb, "estep", tag)
    assert all(e.outside_untouched() for e in (el, e1, eb)) and _unchanged(ops), tag


def _check_e(c, ref, el, e1, eb, entry, tag):
    F = R.tile(c, ref["F"])
    fmax = np.abs(F).max(axis=1)
    assert el.written() and e1.written() and eb.written(), tag
    _close_rows(el.host(), F, None, entry, "logpj", c["hot"], tag)
    _close_rows(e1.host()[0], R.tile(c, ref["lse1"]), fmax, entry, "lse1", c["hot"], tag)
    _close_rows(eb.host()[0], R.tile(c, ref["lseb"]), fmax, entry, "lseb", c["hot"], tag)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_estep(dev, name):
    """DPL 1 / 2 / 4 / 8 / 16, the rho = 21, rho = 6 (either sign) and table powers, S of 0, 1, 2, 3, 63, 64, 65, 129, three
    state tables, H' of 1 .. 16, H of 70 and 130, the second trip of the datapoint loop (u_trip2, s_trip2)."""
    for hot in (True, False):
        c, ref = _case(name, hot)
        for det in (False, True):
            _assert_cell(det, R.ESTEP, c)
            for layout in _layouts(name) if not det else ["odd"]:
                _run_estep(dev, det, c, ref, layout)


# ------------------------------------------------------------------------------------------------ pm_mca_mstep_rows_f64
def _run_mstep(dev, det, c, F_in, l1_in, lb_in, cut, layout, tag, zero_start=False):
    """The two-pass M-step on the log-joints and log-evidences GIVEN (the reference's, rounded): its own arithmetic alone."""
    H, D, Hp, S, N = c["H"], c["D"], c["Hp"], c["S"], c["N"]
    ops = _inputs(dev, c, layout)
    for k in ("scores", "wn", "yn"):
        del ops[k]
    K = 1 + H + S
    ops["F"] = Emb(F_in, _ld(K, layout, 2), dev)
    ops["l1"], ops["lb"] = Emb(l1_in, N, dev), Emb(lb_in, N, dev)
    with np.errstate(invalid="ignore"):
        keep = np.asarray(lb_in >= cut)
    # reference from the same float64 inputs, over the distinct rows where the case is periodic
    periodic = c["rows"] < N and np.array_equal(F_in, R.tile(c, F_in[:c["rows"]])) and \
        np.array_equal(lb_in, R.tile(c, lb_in[:c["rows"]]), equal_nan=True)
    if periodic:
        r = slice(0, c["rows"])
        lbk = np.where(keep[r], lb_in[r], 0.0)
        add, q1, aid = R.packed_stats(c, F_in[r], l1_in[r], lbk, keep[r], mult=R.mult(c), qcut=R.QCUT, rows=r)
        q1 = R.tile(c, q1)
        canc = R.sigma_cancellation(c, F_in[r], R.posteriors(c, F_in[r], lbk, R.QCUT), singles=True)
        canc = float((canc * np.where(keep[r], R.mult(c), 0)).sum())
    else:
        lbk = np.where(keep, lb_in, 0.0)
        add, q1, aid = R.packed_stats(c, F_in, l1_in, lbk, keep, qcut=R.QCUT)
        canc = float(R.sigma_cancellation(c, F_in, R.posteriors(c, F_in, lbk, R.QCUT), singles=True)[keep].sum())
    start = _stats_start(H, D, det) * (0.0 if zero_start else 1.0)
    widen = 0.0
    if det:
        widen = (N + 1) * _install_quanta(c, start[:len(add)] + add, float(np.abs(aid).max(initial=0.0))) / 2
    eq, est = Emb(np.zeros((N, H)), _ld(H, layout, 0), dev, fill=False), Emb(start, len(start), dev)
    P = _params(c)
    rc = _lib_of(det).pm_mca_mstep_rows_f64(ops["F"].ptr, ops["F"].ld, ops["l1"].ptr, ops["lb"].ptr, ctypes.c_double(cut),
                                            ops["Y"].ptr, ops["Y"].ld, ops["Wrho"].ptr, ops["Wrm1"].ptr, ops["cand"].ptr,
                                            _mptr(ops), S, ctypes.byref(P), N, H, D, Hp, eq.ptr, eq.ld, est.ptr, _stream())
    torch.cuda.synchronize()
    assert rc == 0, tag
    got_q = eq.host()
    assert eq.written(), tag
    assert not got_q[~keep].any(), (tag, "cut rows are not zero")
    _close_rows(got_q, q1, None, "mstep_rows", "q1", c["hot"], tag)
    if not keep.any():
        assert est.unchanged(), (tag, "nothing kept, but the statistics changed")
    _check_stats(est.host()[0], start, add, c, widen, "mstep_rows", tag, sigma_extra=4 * canc)
    assert eq.outside_untouched() and est.outside_untouched() and _unchanged(ops), tag
    return keep, est.host()[0], add


def _mstep_inputs(c, ref):
    return R.tile(c, ref["F64"]), R.tile(c, ref["lse1_64"]), R.tile(c, ref["lseb_64"])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_mstep_rows(dev, name):
    """HP 4 / 8 / 12 / 16 x both signs x the DPL each tile allows; the multi-slab walks (D of 129 and 257 at H' = 13, 257 and
    513 at H' = 9, 513 at H' = 4, 1024 at H' = 16): scalars, q1 and q1sum are added by the first slab alone -- the statistics
    start non-zero, a second addition doubles a term.  lse_cut below all, above all (zero rows, `stats` bit-unchanged) and
    equal to one datapoint's lseb, which is kept, with a NaN lseb beside it, which is dropped."""
    for hot in (True, False):
        c, ref = _case(name, hot)
        F_in, l1_in, lb_in = _mstep_inputs(c, ref)
        tie = lb_in.copy()
        if c["N"] > 2:
            tie[1] = np.nan
        cut_tie = float(np.sort(lb_in[np.arange(c["N"]) != 1])[c["N"] // 2]) if c["N"] > 2 else float(lb_in[0])
        for det in (False, True):
            _assert_cell(det, R.MSTEP_ROWS, c)
            for layout in _layouts(name) if not det else ["odd"]:
                tag = (name, hot, det, layout, "mstep_rows")
                _run_mstep(dev, det, c, F_in, l1_in, lb_in, -np.inf, layout, tag + ("all",))
                if layout != "tight":
                    continue
                _run_mstep(dev, det, c, F_in, l1_in, lb_in, float(np.max(lb_in)) + 1.0, layout, tag + ("none",))
                keep = _run_mstep(dev, det, c, F_in, l1_in, tie, cut_tie, layout, tag + ("tie",))[0]
                assert keep[np.nonzero(tie == cut_tie)[0]].all() and (c["N"] <= 2 or not keep[1])
                assert c["N"] <= 2 or 0 < keep.sum() < c["N"]


@pytest.mark.parametrize("name,live", [("u_s129", (67,)), ("u_s129", (2,)), ("u_s129", (0, 1, 5)), ("u_s65", (64,)),
                                       ("s_p12_2", (1, 40, 82)), ("u_hp16", (3, 4, 29)), ("s_p12_2", ())])
def test_mstep_rows_live_states(dev, name, live):
    """Live states (beta f_s - lseb > -745.2) only in the second 64-batch, exactly one, an odd number (the last pair's second
    member is then a repeat of the first), none at all: every other multi-cause log-joint is lowered by 3000 T."""
    for hot in (True, False):
        c, ref = _case(name, hot)
        F_in, l1_in, lb_in = _mstep_inputs(c, ref)
        F_in = F_in.copy()
        dead = np.ones(c["S"], dtype=bool)
        dead[list(live)] = False
        F_in[:, 1 + c["H"]:][:, dead] -= 3000.0 * c["T"]
        dl = c["beta"] * F_in[:, 1 + c["H"]:].astype(LD) - lb_in[:, None]
        assert (dl[:, dead] < R.QCUT).all()
        if hot:
            assert (dl[:, ~dead] > R.QCUT).all()
        for det in (False, True):
            _run_mstep(dev, det, c, F_in, l1_in, lb_in, -np.inf, "odd", (name, live, hot, det))


@pytest.mark.parametrize("name", ["u_trip2", "s_trip2"])
def test_mstep_rows_second_trip_state(dev, name):
    """A wavefront's second datapoint (n >= 8192) after a first one with live states has none, and the other way round: V,
    `staged`, `touched` and the cached prefix of the first must not leak into the second."""
    c, ref = _case(name, True)
    assert _assert_cell(False, R.MSTEP_ROWS, c)[6] == 2048
    F_in, l1_in, lb_in = _mstep_inputs(c, ref)
    for first_live in (True, False):
        lb = lb_in.copy()
        lift = np.arange(c["N"]) >= 8192 if first_live else np.arange(c["N"]) < 8192
        lb[lift] += 800.0                       # every weight of these datapoints underflows: no live state, q1 = 0
        _run_mstep(dev, False, c, F_in, l1_in, lb, -np.inf, "odd", (name, first_live))


def test_mstep_rows_elementwise(dev):
    """W_new = Wp / Wq is an element-wise ratio: an element can be dominated by a state of vanishing posterior (the comment
    above `qcut` in mca_mstep_rows_kernel).  Here, with rho = 21, column 1 of the candidates c0 and c2 holds W = 1e-4 and
    that of c1 holds W = 1e3: in the likely states {c0, c1}, {c1, c2} the factor (W_hd / Wbar_sd)^20 of c0 / c2 is 1e-140,
    in the state {c0, c2}, whose posterior is e^-300 .. e^-321, it is 2^-20/21 -- so Wq_m[c0, 1], Wq_m[c2, 1] and their Wp_m are
    the rare state's terms (about 1e-131), 1e9 times what the likely states add.  The statistics start at zero and every
    non-zero element of Wp_m and Wq_m is compared relative to ITS OWN reference value (all addends are >= 0: y >= 0).
    Bound, derived: an addend is q * pow * Wrm1 [* y].  q = exp(beta f - lseb): the argument is formed in float64 from
    |beta f| <= 330 and |lseb| <= 1, so it carries at most (330 + 1 + 1) u of absolute error, which exp turns into that
    relative error, plus exp's own (<= 2.3e-16 as pm_exp_tab documents; libm's is below it); the power 3e-16 (pm_pow_m20_21,
    pm_common.h); two or three products 3 u; the N S = 12 non-negative addends of an element are summed with at most 12 u
    more.  Sum: 332 u + 2.3e-16 + 3e-16 + 15 u = 3.9e-14; applied with the factor 4 of tests/test_dsc_kernels_gpu.py:
    1.6e-13.  Default library only: the deterministic build rounds every addend to a quantum that such an element lies
    below by construction."""
    H, D, Hp, N, S = 4, 3, 3, 4, 3
    W = np.array([[1.0, 1e3, 0.7], [0.9, 1.1, 1.3], [0.5, 1e-4, 0.8], [1.2, 1e-4, 0.6]])
    wrho, wrm1, wn = R.tables(W, 21.0, 0)
    rng = np.random.RandomState(5)
    Y = rng.uniform(0.2, 1.5, size=(N, D))
    c = dict(name="elementwise", hot=False, H=H, D=D, Hp=Hp, S=S, N=N, rows=N, signed=0, T=1.0, rho=21.0, inv_rho=1.0 / 21.0,
             beta=1.0, kind="comb", W=W, Y=Y, cand=np.tile(np.array([2, 0, 3], dtype=np.int32), (N, 1)),
             masks=np.array([3, 5, 6], dtype=np.uint16), Wrho=wrho, Wrm1=wrm1, wnorm2=wn, ynorm2=(Y * Y).sum(axis=1),
             scores=Y @ W.T, pil_bar=-1.0, pre1=-0.5, cells={R.MSTEP_ROWS: (1, 4, 21, 0, 512, 1, 1)})
    _assert_cell(False, R.MSTEP_ROWS, c)
    F = np.empty((N, 1 + H + S))
    F[:, 0] = -3.0
    F[:, 1:1 + H] = -2.0 - 0.1 * np.arange(H)[None, :]
    F[:, 1 + H:] = np.array([-0.5, -300.0, -1.0])[None, :]
    F[:, 1 + H + 1] -= 7.0 * np.arange(N)
    l1, lb = R.lse(F, 1.0)
    l1, lb = l1.astype(np.float64), lb.astype(np.float64)
    _, got, add = _run_mstep(dev, False, c, F, l1, lb, -np.inf, "odd", ("elementwise",), zero_start=True)
    HD = H * D
    want, have = add[HD:3 * HD], got[HD:3 * HD].astype(LD)
    rare = [2 * D + 1, 3 * D + 1, HD + 2 * D + 1, HD + 3 * D + 1]        # Wp_m, Wq_m at (c0, 1) and (c2, 1)
    assert all(1e-140 < float(want[i]) < 1e-125 for i in rare), [float(want[i]) for i in rare]
    nz = want != 0
    rel = np.abs(have[nz] - want[nz]) / want[nz]
    bound = 4 * (332 * 2.0 ** -53 + 2.3e-16 + 3e-16 + 15 * 2.0 ** -53)
    print("worst element-wise error of Wp_m / Wq_m, two-pass M-step: %.3e (bound %.3e)" % (float(rel.max()), bound))
    assert float(rel.max()) <= bound, (float(rel.max()), bound, np.nonzero(nz)[0][int(np.argmax(rel))])
    assert np.array_equal(have[~nz], np.zeros(int((~nz).sum())))


# ------------------------------------------------------------ pm_mca_estep_mstats_f64, pm_mca_estep_mstats_defer_f64 + apply
def _fused_call(lib, ops, c, el, e1, eb, eq, est, erec, esc, P=None):
    H, D, Hp, S, N = c["H"], c["D"], c["Hp"], c["S"], c["N"]
    P = P or _params(c)
    head = (ops["scores"].ptr, ops["scores"].ld, ops["wn"].ptr, ops["yn"].ptr, ops["Y"].ptr, ops["Y"].ld, ops["Wrho"].ptr,
            ops["Wrm1"].ptr, ops["cand"].ptr, _mptr(ops), S, ctypes.byref(P), N, H, D, Hp, el.ptr, el.ld, e1.ptr, eb.ptr,
            eq.ptr, eq.ld, est.ptr)
    if erec is None and esc is None:
        return lib.pm_mca_estep_mstats_f64(*head, _stream())
    return lib.pm_mca_estep_mstats_defer_f64(*head, erec.ptr if erec is not None else None,
                                             esc.ptr if esc is not None else None, _stream())


def _outputs(dev, c, layout, det):
    H, D, Hp, S, N = c["H"], c["D"], c["Hp"], c["S"], c["N"]
    K = 1 + H + S
    start = _stats_start(H, D, det)
    return (Emb(np.zeros((N, K)), _ld(K, layout, 2), dev, fill=False), Emb(np.zeros(N), N, dev, fill=False),
            Emb(np.zeros(N), N, dev, fill=False), Emb(np.zeros((N, H)), _ld(H, layout, 0), dev, fill=False),
            Emb(start, len(start), dev), start)


def _run_fused(dev, det, c, ref, fr, layout):
    H, D, N = c["H"], c["D"], c["N"]
    add, q1, rec, sc, canc = fr
    ops = _inputs(dev, c, layout)
    el, e1, eb, eq, est, start = _outputs(dev, c, layout, det)
    widen = 0.0
    if det:
        widen = (N + 1) * _install_quanta(c, start[:len(add)] + add, float(np.abs(rec).max(initial=0.0))) / 2
    rc = _fused_call(_lib_of(det), ops, c, el, e1, eb, eq, est, None, None)
    torch.cuda.synchronize()
    tag = (c["name"], c["hot"], det, layout, "fused")
    assert rc == 0, tag
    _check_e(c, ref, el, e1, eb, "fused", tag)
    assert eq.written(), tag
    _close_rows(eq.host(), R.tile(c, q1), None, "fused", "q1", c["hot"], tag)
    _check_stats(est.host()[0], start, add, c, widen, "fused", tag, sigma_extra=4 * float((canc * R.mult(c)).sum()))
    assert all(e.outside_untouched() for e in (el, e1, eb, eq, est)) and _unchanged(ops), tag


def _run_defer(dev, det, c, ref, fr, layout, cuts):
    H, D, Hp, N = c["H"], c["D"], c["Hp"], c["N"]
    _, q1, rec, sc, canc = fr
    lib = _lib_of(det)
    ops = _inputs(dev, c, layout)
    el, e1, eb, eq, est, start = _outputs(dev, c, layout, det)
    erec, esc = Emb(np.zeros((N, Hp * D)), Hp * D, dev, fill=False), Emb(np.zeros((N, 4)), 4, dev, fill=False)
    if det:
        _install_quanta(c, start, float(np.abs(rec).max(initial=0.0)))
    rc = _fused_call(lib, ops, c, el, e1, eb, eq, est, erec, esc)
    torch.cuda.synchronize()
    tag = (c["name"], c["hot"], det, layout, "defer")
    assert rc == 0, tag
    _check_e(c, ref, el, e1, eb, "defer", tag)
    assert est.unchanged(), (tag, "the deferred pass accumulated into the statistics")
    assert eq.written() and erec.written() and esc.written(), tag
    _close_rows(eq.host(), R.tile(c, q1), None, "defer", "q1", c["hot"], tag)
    got_rec, got_sc = erec.host(), esc.host()
    _close_rows(got_rec, R.tile(c, rec.reshape(c["rows"], -1)), None, "defer", "records", c["hot"], tag)
    if c["S"] == 0:
        assert not got_rec.any(), (tag, "S = 0: zero records")
    assert not got_sc[:, 3].any(), (tag, "defer_sc[3]")
    scw = R.tile(c, sc)
    for k, what in enumerate(("sc.pi", "sc.sigma", "sc.lse1")):
        _close_rows(got_sc[:, k], scw[:, k], np.abs(R.tile(c, ref["F"])).max(axis=1) if k == 2 else None, "defer", what, c["hot"], tag,
                    extra=4 * R.tile(c, canc) if k == 1 else 0.0)
    assert all(e.outside_untouched() for e in (el, e1, eb, eq, est, erec, esc)) and _unchanged(ops), tag
    # ... then the kept datapoints' statistics, the cut a device double: none kept, all kept, half kept with a tie
    lb_out = eb.host()[0].copy()
    q1_out = eq.host().copy()
    wlen = int(lib.pm_mca_defer_apply_work_len(H, D))
    _assert_plan_apply(det, c)
    for how in cuts:
        cut = {"none": float(lb_out.max()) + 1.0, "all": -np.inf, "tie": float(np.sort(lb_out)[N // 2])}[how]
        keep = lb_out >= cut
        assert {"none": not keep.any(), "all": keep.all(), "tie": keep.any() and (N < 3 or not keep.all())}[how]
        r = slice(0, c["rows"])
        if c["rows"] < N:
            keep_r = keep[:c["rows"]]
            assert np.array_equal(keep, R.tile(c, keep_r)), "the kernel's lseb is periodic with the rows"
            add, _, _ = R.packed_stats(c, ref["F"], ref["lse1"], ref["lseb"], keep_r, mult=R.mult(c), rows=r)
            cs = float((canc * np.where(keep_r, R.mult(c), 0)).sum())
        else:
            add, _, _ = R.packed_stats(c, ref["F"], ref["lse1"], ref["lseb"], keep)
            cs = float(canc[keep].sum())
        widen = 0.0
        if det:
            widen = (N + 1) * _install_quanta(c, start[:len(add)] + add, float(np.abs(rec).max(initial=0.0))) / 2
        ecut, ework = Emb(np.array([cut]), 1, dev), Emb(np.zeros(wlen), wlen, dev, fill=False)
        ins = dict(ops, lb=Emb(lb_out, N, dev), rec=Emb(got_rec, Hp * D, dev), sc=Emb(got_sc, 4, dev), cut=ecut)
        eq2, est2 = Emb(q1_out, eq.ld, dev), Emb(start, len(start), dev)
        rc = lib.pm_mca_defer_apply_f64(ins["lb"].ptr, ecut.ptr, ins["Y"].ptr, ins["Y"].ld, ins["cand"].ptr, ins["rec"].ptr,
                                        ins["sc"].ptr, eq2.ptr, eq2.ld, est2.ptr, ework.ptr, N, H, D, Hp, _stream())
        torch.cuda.synchronize()
        t2 = tag + (how,)
        assert rc == 0, t2
        assert np.array_equal(eq2.host(), np.where(keep[:, None], q1_out, 0.0)), (t2, "q1 rows")
        _check_stats(est2.host()[0], start, add, c, widen, "defer+apply", t2, sigma_extra=4 * cs)
        assert eq2.outside_untouched() and est2.outside_untouched() and ework.outside_untouched() and _unchanged(ins), t2


def _assert_plan_apply(det, c):
    rc, p = _plan(det, R.DEFER_APPLY, c)
    assert rc == PM_OK and p[0] == c["cells"][R.FUSED][0] and (c["N"] <= 8192 or p[14] == 2048), p


@pytest.mark.parametrize("name", FUSED_NAMES)
def test_fused(dev, name):
    """pm_mca_estep_mstats_f64: each of the ten (DPL, HP) tiles for unsigned W, signed W at rho = 6 and signed W at rho = 13/3
    (tests/test_mca_kernels_cpu.py::test_table_covers_every_cell asserts that the table holds all thirty cells), the PAIRED
    form (signed W, tiles (12, 2), (8, 4), (12, 4)) with odd S, S = 1, S = 2, S = 3, signed W with exact cancellations (t = 0),
    the second trip of the datapoint loop.  H' at the tile's height and at the previous height + 1, and D at the top and at
    the bottom of a DPL, are each reached for every tile height and every DPL, not for each of the thirty cells."""
    for hot in (True, False):
        c, ref = _case(name, hot)
        fr = _fused_ref(name, hot)
        for det in (False, True):
            _assert_cell(det, R.FUSED, c, 0)
            for layout in _layouts(name) if not det else ["odd"]:
                _run_fused(dev, det, c, ref, fr, layout)


@pytest.mark.parametrize("name", FUSED_NAMES)
def test_fused_deferred(dev, name):
    """pm_mca_estep_mstats_defer_f64 (records and scalars compared directly, nothing accumulated) + pm_mca_defer_apply_f64
    over {none kept, all kept, half kept with a tie at the cut}."""
    for hot in (True, False):
        c, ref = _case(name, hot)
        fr = _fused_ref(name, hot)
        for det in (False, True):
            _assert_cell(det, R.FUSED, c, 1)
            for layout in (_layouts(name) if not det else ["odd"]):
                _run_defer(dev, det, c, ref, fr, layout, ("none", "all", "tie") if layout != "tight" else ("tie",))


@pytest.mark.parametrize("defer", [False, True])
def test_fused_elementwise(dev, defer):
    """The situation of test_mstep_rows_elementwise for the fused pass, in-pass and deferred + pm_mca_defer_apply_f64, from
    DATA (these entries form their own log-joints): rho = 21, column 1 of c0 and c2 holds 1e-4 and that of c1 holds 1e3, every
    datapoint is Wbar of {c0, c1} plus noise in [0, 0.3], pre1 = -3e-4.  States without c1 miss y_1 = 1e3 by an energy of 1e6:
    {c0, c2} has a posterior of e^-300, and its factor 2^-20/21 at (c0, 1) and (c2, 1) outweighs the likely states' 1e-140
    by 1e9.  Statistics start at zero; every non-zero element of Wp_m / Wq_m is compared relative to its own reference value.
    Bound, derived.  An addend is w g fac [y] with w = exp(beta f - M), g = exp(M - lseb).  beta f of the rare state is -300:
    the kernel's own f = pil_bar |s| + pre1 sum_d (Wbar - y)^2 carries a subtraction, a square and D = 3 additions per term,
    the product with pre1 and the sum with the prior -- at most 8 u |f|; the two exponents beta f - M and M - lseb round once
    each on magnitudes <= 330: 2 * 330 u; lseb itself (|lseb| < 5, a sum of 8 terms): 12 u; two exponentials 2 * 2.3e-16
    (pm_exp_tab, pm_common.h), the power 5e-16 (pm_pow_uni), four products 4 u, at most N S = 12 non-negative addends 12 u.
    Sum: (8 * 330 + 660 + 28) u + 9.6e-16 = 3.7e-13; with the factor 4 of tests/test_dsc_kernels_gpu.py: 1.5e-12.  Default
    library only (the deterministic build rounds addends to a quantum such an element lies below)."""
    H, D, Hp, N, S = 4, 3, 3, 4, 3
    W = np.array([[1.0, 1e3, 0.7], [0.9, 1.1, 1.3], [0.5, 1e-4, 0.8], [1.2, 1e-4, 0.6]])
    wrho, wrm1, wn = R.tables(W, 21.0, 0)
    rng = np.random.RandomState(11)
    Y = (wrho[2] + wrho[0]) ** (1.0 / 21.0) + rng.uniform(0.0, 0.3, size=(N, D))
    c = dict(name="elementwise_fused", hot=False, H=H, D=D, Hp=Hp, S=S, N=N, rows=N, signed=0, T=1.0, rho=21.0,
             inv_rho=1.0 / 21.0, beta=1.0, kind="comb", W=W, Y=Y, cand=np.tile(np.array([2, 0, 3], dtype=np.int32), (N, 1)),
             masks=np.array([3, 5, 6], dtype=np.uint16), Wrho=wrho, Wrm1=wrm1, wnorm2=wn,
             ynorm2=(Y.astype(LD) ** 2).sum(axis=1).astype(np.float64), scores=(Y.astype(LD) @ W.astype(LD).T).astype(np.float64),
             pil_bar=-1.0, pre1=-3e-4, cells={R.FUSED: (1, 4, 0, 0)})
    _assert_cell(False, R.FUSED, c, int(defer))
    ref = R.case_reference(c)
    dl = ref["F"][:, 1 + H:] - ref["lseb"][:, None]
    assert (dl[:, 1] < -250).all() and (dl[:, 1] > -330).all() and (dl[:, 0] > -3).all() and np.abs(ref["lseb"]).max() < 5
    add, _, _ = R.packed_stats(c, ref["F"], ref["lse1"], ref["lseb"], np.ones(N, dtype=bool))
    lib = _lib_of(False)
    ops = _inputs(dev, c, "odd")
    el, e1, eb, eq, _, start = _outputs(dev, c, "odd", False)
    est = Emb(start * 0.0, len(start), dev)
    if not defer:
        assert _fused_call(lib, ops, c, el, e1, eb, eq, est, None, None) == 0
    else:
        erec, esc = Emb(np.zeros((N, Hp * D)), Hp * D, dev, fill=False), Emb(np.zeros((N, 4)), 4, dev, fill=False)
        assert _fused_call(lib, ops, c, el, e1, eb, eq, est, erec, esc) == 0
        wlen = int(lib.pm_mca_defer_apply_work_len(H, D))
        ecut, ework = Emb(np.array([-np.inf]), 1, dev), Emb(np.zeros(wlen), wlen, dev, fill=False)
        assert lib.pm_mca_defer_apply_f64(eb.ptr, ecut.ptr, ops["Y"].ptr, ops["Y"].ld, ops["cand"].ptr, erec.ptr, esc.ptr, eq.ptr,
                                          eq.ld, est.ptr, ework.ptr, N, H, D, Hp, _stream()) == 0
    torch.cuda.synchronize()
    got = est.host()[0]
    HD = H * D
    want, have = add[HD:3 * HD], got[HD:3 * HD].astype(LD)
    rare = [2 * D + 1, 3 * D + 1, HD + 2 * D + 1, HD + 3 * D + 1]        # Wp_m, Wq_m at (c0, 1) and (c2, 1)
    assert all(1e-145 < float(want[i]) < 1e-105 for i in rare), [float(want[i]) for i in rare]
    likely, _, _ = R.packed_stats(dict(c, masks=np.array([3, 0, 6], dtype=np.uint16)), ref["F"], ref["lse1"], ref["lseb"],
                                  np.ones(N, dtype=bool))
    assert all(float(likely[HD:3 * HD][i]) < 1e-6 * float(want[i]) for i in rare), "the rare state dominates these elements"
    nz = want != 0
    rel = np.abs(have[nz] - want[nz]) / want[nz]
    bound = 4 * ((8 * 330 + 660 + 28) * 2.0 ** -53 + 9.6e-16)
    print("worst element-wise error of Wp_m / Wq_m, fused pass%s: %.3e (bound %.3e)" % (" deferred + apply" if defer else "",
                                                                                      float(rel.max()), bound))
    assert float(rel.max()) <= bound, (float(rel.max()), bound, np.nonzero(nz)[0][int(np.argmax(rel))])
    assert not have[~nz].any() and est.outside_untouched() and _unchanged(ops)


@pytest.mark.parametrize("name", list(R.RESCALE))
def test_fused_rescale(dev, name):
    """The reference level of the fused pass moves (`bf > M + 50`) at the states the table's order sets (module docstring),
    in-pass and deferred, both libraries."""
    c, ref = _case(name, True)
    fr = _fused_ref(name, True)
    assert R.rescale_points(c, ref) == R.RESCALE[name][2], name
    for det in (False, True):
        _assert_cell(det, R.FUSED, c, 0)
        _run_fused(dev, det, c, ref, fr, "odd")
        _run_defer(dev, det, c, ref, fr, "tight", ("all",))


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_outputs_alone(dev):
    """PM_ERANGE at D = 1025, H' = 17, H' > H, S = 65536 (E-step); D = 513, H' = 13, (D = 257, H' = 5), H' > H (fused, both
    forms); H' = 17, H' > H (two-pass M-step); PM_EINVAL for one-sided defer_rec / defer_sc: every output keeps its pattern."""
    base, ref = _case("u_d65", True)
    for det in (False, True):
        lib = _lib_of(det)
        for entry, over, want in (("estep", dict(D=1025), PM_ERANGE), ("estep", dict(Hp=17, H=20), PM_ERANGE),
                                  ("estep", dict(Hp=8), PM_ERANGE), ("estep", dict(S=65536), PM_ERANGE),
                                  ("fused", dict(D=513), PM_ERANGE), ("fused", dict(Hp=13, H=20), PM_ERANGE),
                                  ("fused", dict(D=257, Hp=5), PM_ERANGE), ("fused", dict(Hp=8), PM_ERANGE),
                                  ("defer", dict(D=513), PM_ERANGE), ("defer", dict(Hp=13, H=20), PM_ERANGE),
                                  ("defer", dict(D=257, Hp=5), PM_ERANGE), ("defer", dict(Hp=8), PM_ERANGE),
                                  ("rec_only", dict(), PM_EINVAL), ("sc_only", dict(), PM_EINVAL),
                                  ("mstep", dict(Hp=17, H=20), PM_ERANGE), ("mstep", dict(Hp=8), PM_ERANGE)):
            c = dict(base)
            c.update(over)
            H, D, Hp, S, N = c["H"], c["D"], c["Hp"], c["S"], 4
            c["N"] = N
            # operands of the claimed shape (zeros: never read); the state table of S = 65536 masks is real too
            z = dict(scores=np.zeros((N, H)), wnorm2=np.zeros(H), ynorm2=np.zeros(N), Y=np.zeros((N, D)), Wrho=np.ones((H, D)),
                     Wrm1=np.ones((H, D)), cand=np.tile(np.arange(Hp, dtype=np.int32) % H, (N, 1)),
                     masks=np.full(S, 3, dtype=np.uint16))
            c.update(z)
            ops = _inputs(dev, c, "odd")
            el, e1, eb, eq, est, start = _outputs(dev, c, "odd", det)
            erec, esc = Emb(np.zeros((N, Hp * D)), Hp * D, dev, fill=False), Emb(np.zeros((N, 4)), 4, dev, fill=False)
            P = _params(c)
            if entry == "estep":
                rc = lib.pm_mca_estep_f64(ops["scores"].ptr, ops["scores"].ld, ops["wn"].ptr, ops["yn"].ptr, ops["Y"].ptr,
                                          ops["Y"].ld, ops["Wrho"].ptr, ops["cand"].ptr, _mptr(ops), S, ctypes.byref(P), N, H, D,
                                          Hp, el.ptr, el.ld, e1.ptr, eb.ptr, _stream())
            elif entry == "mstep":
                fin = Emb(np.zeros((N, 1 + H + S)), 1 + H + S, dev)
                lin = Emb(np.zeros(N), N, dev)
                rc = lib.pm_mca_mstep_rows_f64(fin.ptr, fin.ld, lin.ptr, lin.ptr, ctypes.c_double(-1.0), ops["Y"].ptr, ops["Y"].ld,
                                               ops["Wrho"].ptr, ops["Wrm1"].ptr, ops["cand"].ptr, _mptr(ops), S, ctypes.byref(P), N,
                                               H, D, Hp, eq.ptr, eq.ld, est.ptr, _stream())
            else:
                rc = _fused_call(lib, ops, c, el, e1, eb, eq, est, erec if entry in ("defer", "rec_only") else None,
                                 esc if entry in ("defer", "sc_only") else None, P)
            torch.cuda.synchronize()
            tag = (entry, over, det)
            assert rc == want, (tag, rc)
            which = {"estep": R.ESTEP, "mstep": R.MSTEP_ROWS}.get(entry, R.FUSED)
            if want == PM_ERANGE:
                assert _plan(det, which, c)[0] == PM_ERANGE, (tag, "the plan refuses what the launcher refuses")
            assert all(e.unchanged() for e in (el, e1, eb, eq, est, erec, esc)) and _unchanged(ops), tag


@pytest.fixture(scope="module", autouse=True)
def _report_worst_errors():
    """After the module's tests: the largest error of every bounded comparison that ran, per entry, quantity and HOT / COLD
    (-s shows it).  Not a check of its own: each comparison asserted its bound where it was made."""
    yield
    for key in sorted(WORST):
        ratio, err, bound = WORST[key]
        print("worst %-12s %-12s %-4s err %.3e  bound %.3e  ratio %.3f" % (key + (err, bound, ratio)))
