"""The 16-wavefront Binary Sparse Coding E-step (bsc_fused8.hip) through the C ABI -- pm_bsc_estep_fused8_f64, _nz_f64,
_defer_f64 and pm_bsc_defer_apply_f64 -- on padded, guarded operands, one smallest shape per instantiation
<HP, GAMMA, FULL, MSTATS, TAIL> of bsc_estep_fused8s_kernel (64 cells, each confirmed with pm_bsc_plan inside the test, with
the device's CU count), against the plain NumPy reference tests/bsc_kernels_reference.py, from both libraries.  The same for
the other launchers, one case per plan cell (second half of the module): pm_bsc_estep_f64 and pm_bsc_mstep_rows_f64,
pm_bsc_select_estep_f64 at every VPL boundary and one past it (mode 1, 2, 3 and the ranking bits 2, 3, 4),
pm_bsc_mstep_rows16_f64 / _nz_f64 (plain and lists, rows with exactly 16 and with 17 non-zeros, cut rows, the row whose lse
equals the cut), pm_bsc_estep_fused_f64 (NJ 8 and 16, FULL and not, with and without statistics, N around the 64-row tile, D
around the ring depth, D_stats > D); and, with integer operands and equality, pm_bsc_select_f64 on both sides of every VPL
switch and the five sparse products of bsc_wp_sparse.hip.  tests/test_bsc_kernels_cpu.py sweeps pm_bsc_plan over every H and
fails if a cell has no case.

Harness: ``Emb`` of tests/test_eval_kernels_gpu.py with the uint16 extension of tests/test_dsc_kernels_gpu.py (16 guard rows
before and after, padding columns, a quiet-NaN payload / 0xDEADBEEF / 0xA5A5 pattern).  After every call the result block
equals the reference, every guard and padding element of every output still holds the pattern, every input is bit-unchanged.
cand, state_masks, state_parents, nz_idx and the statistics start at odd element offsets; Y and Wt stay 16-byte aligned with
even leading dimensions (the PM_EINVAL of the misaligned call is tested instead); logpj and E[s] rows are padded.

Exact arithmetic (bsc_kernels_reference.make_case; tests/test_bsc_kernels_cpu.py asserts it for every case).  Y, Wt and mu are
small integers, |W_h|^2 a power of 4, ecoef -2 or -2^-20, prior_scale 1 or 1/2, pil_bar a multiple of 2^-4: scores, Gram
entries and energies are integers far below 2^53 in any summation order, the ranking key a / |W_h| has fewer than 32
significant bits, ecoef e + prior is exact with or without a fused multiply-add, on the incremental parent-plus-delta walk
too.  Candidates (every case has real ties at the H' boundary: equal rows of W), log-joints, list indices, overflow and kept
counts, and the rows a call must not write are compared with equality.  lse against bsc_kernels_reference.lse_bound (derived
there; its lanes per datapoint: 32 in bsc_fused8.hip, 64 in the wavefront kernels of bsc_kernels.hip, 16 in the sixteen-lane
passes of bsc_rows16.hip and bsc_fused.hip).  Posterior-weighted outputs (E[s], Wq, qdiag, mus, sum q e, list values, records) against the
longdouble reference with RTOL = 1e-11 of tests/test_eval_kernels_gpu.py: row-relative for rows, relative to the largest value
of their section for statistics.  The reference leaves out the weights the kernel documents as left out (f <= max - 37).
Such a bound cannot see a state of weight 1e-12, so every case also runs HOT: ecoef = -2^-20 puts all weights of a row within
a factor e, and a dropped, doubled or misplaced column moves a result by ~1 / K.  The COLD run (ecoef = -2) has terms below the
cut-off, rows with at most PM_BSC_NZ_MAX non-zeros and rows with more.

Deterministic library: quanta of unit `bsc_fused8` per category (0 sums of probabilities, 1 sum q e, 2 sum of lse): the bound
2^k >= 4 (N + 1) max(1, |e|, |lse|) of the category exceeds every partial sum, the quantum is 2^(k - 51).  A statistic receives at
most N + 1 quantised addends, each off by at most quantum / 2: its bound widens by (N + 1) quantum / 2.  Two runs of every
statistics-producing call, on fresh guarded outputs, are bit-identical there -- every fused8 entry, part and mode,
pm_bsc_defer_apply_f64, pm_bsc_mstep_rows_f64, pm_bsc_mstep_rows16_f64 / _nz_f64 and pm_bsc_estep_fused_f64 (_same_bits).

Main-launch cases take N = 2 cus 16 + 1 rows from the plan (8193 at 256 CUs: 64 full tiles and a one-row tile); their rows
repeat with period 67, so the reference is computed on 67 rows.

Mutants of bsc_fused8.hip / bsc_rows16_body.h (one value or predicate each, never an index, bound or address; scratch copies
of the default library, each run once over the 77 tests that use it, MI355X) and the checks that fail:
  `!(l >= cut)` -> `!(l > cut)` in bsc_defer_apply_kernel      4 tests: "a kept row changed" (the hot apply runs whose cut
                                                               equals one row's lse: its list was emptied)
  `2.0 * (G terms)` -> `1.0 *` in the incremental energies     75: logpj of every multi-cause column, first at column 1 + H
  prior_scale ignored in the multi-cause columns               75: logpj of the cold runs (prior_scale = 1/2)
  NEGLIGIBLE -37 -> -3                                         75: lse (off by up to 0.1 against a bound of 1e-13)
  overflow test `nzn > PM_BSC_NZ_MAX` -> `>=`                  1: "the dense row of a complete list was stored"
                                                               (tail_hp6_g4_part_ms, cold: its row with exactly 16 non-zeros)
  qdiag written to the diagonal of the Wq block instead        42: "an entry no datapoint contributes to was written"
  singleton f of a register without a latent -1e300 -> 0       40: lse of every case with H < 256, both launches
The last one stands in for "the shadow rows of H < 256 take their values from row H - 2": in this kernel the shadow rows
are an address clamp of the W loads (rb < H ? rb : H - 1), which a mutant may not touch, and their scores are masked at every
use -- the ranking key (-inf), the singleton log-joint (-1e300) and the predicated stores; the mutant removes the second mask.
None of the seven is equivalent, none survived.  Four more, of the other kernel files, each run once over the default-library
tests of the wave, rows16 and fused entries:
  `l >= lse_cut` -> `l > lse_cut` in bsc_mstep_rows16_kernel   11 (every rows16 case, hot): "expect" -- the row whose lse
                                                               equals the cut became a zero row (row-relative error 1)
  `k >= i` -> `k > i` in its Wq scatter (the diagonal dropped)  11 (every rows16 case): "Wq"
  the diagonal left out of the fused kernel's Wq scatter        4 (the four fused cases with statistics): "Wq"
  `!(l >= lse_cut)` -> `!(l > lse_cut)` in bsc_mstep_rows_kernel  4 (every wave case, hot): "expect", as above"""
import ctypes
import functools

import numpy as np
import pytest

import bsc_kernels_reference as R
from test_dsc_kernels_gpu import Emb, _odd
from test_eval_kernels_gpu import RTOL, _stream, dev, row_rel  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PM_OK, PM_EINVAL, PM_ERANGE = 0, -1, -2
LD = np.longdouble
FUSED8_NAMES = [n for n, s in R.CASES.items() if s["entry"] == "fused8"]
LANES = 32                      # lanes per datapoint of the fused8 row passes


def _lib_of(det):
    from prosper_amd import _lib
    return _lib.load(det)


@functools.lru_cache(maxsize=None)
def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _plan(det, which, c, flags, N=None):
    out = (ctypes.c_int32 * R.PLAN_LEN)(*([-7] * R.PLAN_LEN))
    rc = _lib_of(det).pm_bsc_plan(which, c["H"], c["D"], c["Hp"], c["S"], c["gamma"], flags, c["N"] if N is None else N, 0, out)
    return rc, tuple(out)


@functools.lru_cache(maxsize=None)
def _case(name, hot, given=False):
    """Operands and reference of a case, computed once and shared by every test (and both libraries).  given: the candidates
    are handed in (mode 2) instead of selected."""
    c = R.make_case(name, hot, cus=_cus())
    ref = R.case_reference(c, cand=c["cand_in"] if given else None)
    assert ref["exact"] and (given or ref["boundary_ties"] > 0)
    return c, ref


def _params(c, **over):
    from prosper_amd import _lib
    P = _lib.EStepParams()
    P.pil_bar, P.ecoef, P.prior_scale, P.mu_sqnorm = c["pil_bar"], c["ecoef"], c["prior_scale"], c["mu_sqnorm"]
    for k, v in over.items():
        setattr(P, k, v)
    return P


def _even(n, pad):
    """An even leading dimension >= n (Y and Wt rows stay 16-byte aligned); pad: with padding columns."""
    return n + (2 if pad else 0) + (n % 2)


def _inputs(dev, c, pad):
    H, D, N = c["H"], c["D"], c["N"]
    ops = dict(Y=Emb(c["Y"], _even(D, pad), dev), Wt=Emb(c["Wt"], _even(D, not pad), dev), G=Emb(c["G"], H, dev),
               yn2=Emb(c["yn2"], N, dev), masks=_odd(c["masks"], c["S"], dev), parents=_odd(c["parents"], c["S"], dev))
    if c["mu"] is not None:
        ops["wmu"], ops["ymu"] = Emb(c["wmu"], H, dev), Emb(c["ymu"], N, dev)
    assert ops["Y"].addr % 16 == 0 and ops["Wt"].addr % 16 == 0
    return ops


def _p(ops, k):
    return ops[k].ptr if k in ops else None


def _quanta(c, ref):
    """Quanta of the BSC units in the deterministic library (module docstring); returns the three categories' quanta."""
    from prosper_amd import _lib
    from prosper_amd.em.camodels import _device
    r = c["rows"]
    big = [1.0, max(1.0, float(np.abs(ref["E"][:r]).max())), max(1.0, float(np.abs(ref["lse"][:r]).max()))]
    ks = [int(np.ceil(np.log2(4.0 * (c["N"] + 1) * b))) for b in big]
    M8 = (ctypes.c_double * 8)(*([1.5 * 2.0 ** (k + 1) for k in ks] + [1.5 * 2.0 ** (ks[0] + 1)] * 5))
    for unit in ("bsc_fused8", "bsc_rows16", "bsc_fused", "bsc_kernels"):
        _device._DET_QUANTA_SET.pop(unit, None)
        _lib.call("pm_det_set_quanta", _lib.DET_UNITS[unit], M8, _stream(), det=True)
    torch.cuda.synchronize()
    return [2.0 ** (k - 51) for k in ks]


def _forget_quanta():
    from prosper_amd.em.camodels import _device
    for unit in ("bsc_fused8", "bsc_rows16", "bsc_fused", "bsc_kernels", "wp_sparse"):
        _device._DET_QUANTA_SET.pop(unit, None)


def _stats_start(n):
    """A non-zero start the statistics are accumulated into: position-dependent multiples of 1/8 in [1/8, 1]."""
    return (1 + (np.arange(n) * 5) % 8) / 8.0


def _raw(e):
    """The result block of an Emb as the integers its bits spell."""
    b = e.block().contiguous()
    return (b.view(torch.int64) if b.dtype == torch.float64 else b).cpu().numpy()


def _check_stats(got, start, want, H, D, quanta, N, what):
    """The packed statistics against start + want (longdouble): entries nothing contributes to bit-unchanged, the others
    within RTOL of their section's largest value (+ the deterministic widening of their category)."""
    total = start.astype(LD) + want
    zero = np.asarray(want == 0)
    assert np.array_equal(got[zero], start[zero]), (what, "an entry no datapoint contributes to was written",
                                                    np.nonzero(got[zero] != start[zero])[0][:5].tolist())
    sec = R.stats_sections(H, D)
    sc = sec["scalars"].start
    pieces = [("Wq", sec["Wq"], 0), ("qdiag", sec["qdiag"], 0), ("mus", sec["mus"], 0), ("sum q e", slice(sc, sc + 1), 1),
              ("sum lse", slice(sc + 1, sc + 2), 2)]
    for nm, sl, cat in pieces:
        scale = float(np.abs(total[sl]).max())
        err = float(np.abs(got[sl].astype(LD) - total[sl]).max())
        widen = (N + 1) * quanta[cat] / 2 if quanta else 0.0
        assert err <= RTOL * scale + widen, (what, nm, err, scale, widen)
    assert got[sc + 2] == float(total[sc + 2]) and got[sc + 3] == float(total[sc + 3]), (what, "kept / overflow", got[sc + 2:],
                                                                                        total[sc + 2:])


class Fused8:
    """One call of pm_bsc_estep_fused8_f64 / _nz_f64 / _defer_f64 on guarded operands, and its checks."""

    def __init__(self, dev, det, c, ref, entry="plain", mode=3, part=0, pad=True, stats=None, D_stats=None):
        self.det, self.c, self.ref, self.entry, self.mode, self.part = det, c, ref, entry, mode, part
        H, Hp, S, N, D = c["H"], c["Hp"], c["S"], c["N"], c["D"]
        self.stats = c["stats"] if stats is None else stats
        self.D_stats = D if D_stats is None else D_stats
        self.lists = entry in ("nz", "defer")
        self.ops = _inputs(dev, c, pad)
        K = c["K"]
        cand0 = R.tile(c, ref["cand"]).astype(np.int32)
        self.cand = _odd(cand0, Hp, dev, fill=not (mode & 1))               # an output under mode bit 0, else an input
        self.el = Emb(np.zeros((N, K)), K + (3 if pad else 0), dev, fill=False)
        self.es = Emb(np.zeros(N), N, dev, fill=False)
        self.ee = Emb(np.zeros((N, H)), H + (1 if pad else 0), dev, fill=False)
        self.start = _stats_start(R.stats_len(H, self.D_stats))
        self.est = _odd(self.start, len(self.start), dev)
        self.ei = _odd(np.zeros((N, R.NZ_MAX), dtype=np.uint16), R.NZ_MAX, dev, fill=False)
        self.ev = Emb(np.zeros((N, R.NZ_MAX)), R.NZ_MAX, dev, fill=False)
        self.er = Emb(np.zeros((N, R.DEFER_LD)), R.DEFER_LD, dev, fill=False)
        self.P = _params(c)
        rc, out = _plan(det, R.FUSED8, c, mode | (R.F_STATS if self.stats else 0) | (R.F_LISTS if self.lists else 0))
        assert rc == 0, (c["name"], rc)
        self.plan = out
        main = out[R.O_MAIN_ROWS]
        self.lo, self.hi = (0, N) if part == 0 else (0, main) if part == 1 else (main, N)

    def outputs(self):
        return [self.el, self.es, self.ee, self.est, self.ei, self.ev, self.er] + ([self.cand] if self.mode & 1 else [])

    def call(self, **ov):
        c, ops = self.c, self.ops
        g = lambda k, d: ov.get(k, d)
        st = self.stats
        head = (g("Y", ops["Y"].ptr), g("ldy", ops["Y"].ld), g("Wt", ops["Wt"].ptr), g("ldw", ops["Wt"].ld), ops["G"].ptr,
                ops["yn2"].ptr, g("wmu", _p(ops, "wmu")), g("ymu", _p(ops, "ymu")), g("masks", ops["masks"].ptr),
                ops["parents"].ptr, g("size_off", c["size_off"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), g("S", c["S"]),
                g("gamma", c["gamma"]), g("P", ctypes.byref(self.P)), g("N", c["N"]), g("D", c["D"]), g("H", c["H"]),
                g("Hp", c["Hp"]), g("mode", self.mode), g("cand", self.cand.ptr), g("logpj", self.el.ptr), g("ldl", self.el.ld),
                g("lse", self.es.ptr), g("expect", self.ee.ptr if st else None), g("lde", self.ee.ld),
                g("stats", self.est.ptr if st else None), g("D_stats", self.D_stats))
        lib = _lib_of(self.det)
        nzi = g("nzi", self.ei.ptr if self.lists else None)
        nzv = g("nzv", self.ev.ptr if self.lists else None)
        part = g("part", self.part)
        if self.entry == "plain":
            rc = lib.pm_bsc_estep_fused8_f64(*head, part, _stream())
        elif self.entry == "nz":
            rc = lib.pm_bsc_estep_fused8_nz_f64(*head, nzi, nzv, part, _stream())
        else:
            rc = lib.pm_bsc_estep_fused8_defer_f64(*head, nzi, nzv, g("records", self.er.ptr), part, _stream())
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        return all(e.unchanged() for e in self.outputs()) and all(e.unchanged() for e in self.ops.values()) and \
            (self.mode & 1 or self.cand.unchanged())

    def check(self, what, quanta=None, records=True):
        """Every output of the call against the reference, on the rows [lo, hi) its `part` covers; the other rows, the guards
        and the padding hold the pattern; the inputs are unchanged."""
        c, ref, lo, hi = self.c, self.ref, self.lo, self.hi
        H, Hp, N, D, r = c["H"], c["Hp"], c["N"], c["D"], c["rows"]
        rows = np.arange(lo, hi)
        inside = np.zeros(N, dtype=bool)
        inside[rows] = True
        assert all(e.outside_untouched() for e in self.outputs()), (what, "guard or padding written")
        assert all(e.unchanged() for e in self.ops.values()), (what, "an input changed")

        def only_inside(e, nm):
            raw = _raw(e)
            assert (raw[~inside] == e.sent).all(), (what, nm, "rows outside the part were written")
            return raw
        if self.mode & 1:
            got = self.cand.host()
            only_inside(self.cand, "cand")
            want = R.tile(c, ref["cand"])
            assert np.array_equal(got[rows], want[rows]), (what, "cand", np.argwhere(got[rows] != want[rows])[:5].tolist())
        else:
            assert self.cand.unchanged(), (what, "cand is an input")
        if not self.mode & 2:
            assert all(e.unchanged() for e in (self.el, self.es, self.ee, self.est, self.ei, self.ev, self.er)), what
            return
        F = only_inside(self.el, "logpj").view(np.float64)
        wantF = R.tile(c, ref["F64"])
        assert np.array_equal(F[rows], wantF[rows]), (what, "logpj", np.argwhere(F[rows] != wantF[rows])[:5].tolist())
        lse, raw_lse = self.es.host()[0], _raw(self.es)[0]
        assert (raw_lse[~inside] == self.es.sent).all(), (what, "lse outside the part")
        want_l = R.tile(c, ref["lse"])
        err = np.abs(lse[rows].astype(LD) - want_l[rows])
        bound = R.lse_bound(c["K"], LANES, want_l[rows].astype(np.float64))
        assert (err <= bound).all(), (what, "lse", float(err.max()), float(bound.min()))
        if not self.stats:
            assert all(e.unchanged() for e in (self.ee, self.est, self.ei, self.ev, self.er)), what
            return
        # ---- statistics of the rows [lo, hi): reference on the distinct rows, weighted by their multiplicity in the range
        mult = np.bincount(rows % r, minlength=r)
        drop = R.dropped_onepass(ref["F64"])
        st = R.row_stats(ref["F"], ref["lse"], np.ones(r, dtype=bool), ref["E"], ref["cand"], c["SM"], H, c["ecoef"], mult=mult,
                         drop=drop)
        want_e = R.tile(c, st["expect"])
        over = R.tile(c, st["nz_cnt"]) > R.NZ_MAX
        deferred = self.entry == "defer" and records
        raw_e = _raw(self.ee)
        assert (raw_e[~inside] == self.ee.sent).all(), (what, "expect outside the part")
        exp = raw_e.view(np.float64)
        dense = inside & (over if self.lists else True)
        if dense.any():
            assert row_rel(exp[dense].astype(LD), want_e[dense]) <= RTOL, (what, "expect", row_rel(exp[dense].astype(LD), want_e[dense]))
            assert np.array_equal(exp[dense] == 0, np.asarray(want_e[dense] == 0)), (what, "zeros of expect")
        assert (raw_e[inside & ~dense] == self.ee.sent).all(), (what, "the dense row of a complete list was stored")
        n_over = int((over & inside).sum()) if self.lists else 0
        if deferred:
            zero = dict(st, q1=0 * st["q1"], m1=0 * st["m1"], upper=0 * st["upper"], sig=LD(0), fs=LD(0), cnt=LD(0))
            want_s = R.pack_stats(zero, H, self.D_stats, "fused8", overflow=n_over)
        else:
            want_s = R.pack_stats(st, H, self.D_stats, "fused8", overflow=n_over)
        _check_stats(self.est.host()[0], self.start, want_s, H, self.D_stats, quanta, N, what)
        if self.lists:
            self.check_lists(what, st, inside, over, want_e)
        else:
            assert self.ei.unchanged() and self.ev.unchanged(), what
        if deferred:
            rec = _raw(self.er)
            assert (rec[~inside] == self.er.sent).all() and (rec[:, 37:] == self.er.sent).all(), (what, "records outside")
            got_r, want_r = rec.view(np.float64)[inside][:, :37], R.tile(c, st["records"])[inside][:, :37]
            assert row_rel(got_r[:, :36].astype(LD), want_r[:, :36]) <= RTOL, (what, "records")
            assert np.array_equal(got_r[:, :36] == 0, np.asarray(want_r[:, :36] == 0)), (what, "zeros of the records")
            assert (np.abs(got_r[:, 36].astype(LD) - want_r[:, 36]) <= RTOL * np.abs(want_r[:, 36])).all(), (what, "record q e")
        else:
            assert self.er.unchanged(), what

    def check_lists(self, what, st, inside, over, want_e):
        """nz_idx exactly (ascending non-zero latents, 0xFFFF behind them, PM_BSC_NZ_OVERFLOW in slot 0 of a row with more
        than PM_BSC_NZ_MAX), nz_val against the reference's E[s], slots behind a list never written."""
        c = self.c
        idx = _raw(self.ei).astype(np.int64) & 0xFFFF
        sent = self.ei.sent & 0xFFFF
        assert (idx[~inside] == sent).all(), (what, "nz_idx outside the part")
        want_idx, _ = R.lists_of(R.tile(c, st["expect"]))
        first = want_idx[:, 0].copy()
        want_idx[over, 0] = R.NZ_OVERFLOW
        assert np.array_equal(idx[inside], want_idx[inside]), (what, "nz_idx", np.argwhere(idx[inside] != want_idx[inside])[:5].tolist())
        want_idx[:, 0] = first
        raw_v = _raw(self.ev)
        filled = (want_idx != R.NZ_PAD) & inside[:, None]
        assert (raw_v[~filled] == self.ev.sent).all(), (what, "nz_val written behind a list or outside the part")
        n_i, t_i = np.nonzero(filled)
        got_v = raw_v.view(np.float64)[n_i, t_i].astype(LD)
        want_v = want_e[n_i, want_idx[n_i, t_i]]
        scale = np.abs(want_e).max(axis=1)[n_i]
        assert (np.abs(got_v - want_v) <= RTOL * scale).all(), (what, "nz_val")


def _same_bits(first, second, what):
    """Two runs of a statistics-producing call in the deterministic library: every output element, guards included."""
    for a, b in zip(first, second):
        assert torch.equal(a._raw(), b._raw()), (what, "two runs of the deterministic library differ")


def _bits(*embs):
    return [_raw(e).copy() for e in embs]


# ------------------------------------------------------------------------------------------- the 64 instantiations, + mu
@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
@pytest.mark.parametrize("name", FUSED8_NAMES)
def test_fused8_cell(dev, name, det):
    """One instantiation <HP, GAMMA, FULL, MSTATS, TAIL> (bsc_kernels_reference.CASES), hot and cold: the plan is the cell's
    and sends every row to the launch the case is named after; pm_bsc_estep_fused8_f64 with mode 3 on padded operands
    (tight ones in every fourth hot run); in the deterministic library a second run returns the same bits."""
    spec = R.CASES[name]
    hp, g, full, ms, tail = spec["cell"]
    for hot in (True, False):
        c, ref = _case(name, hot)
        pad = not (hot and FUSED8_NAMES.index(name) % 4 == 0)            # tight operands in every fourth hot run
        run = Fused8(dev, det, c, ref, pad=pad)
        p = run.plan
        assert (p[R.O_FAMILY], p[R.O_NJ], p[R.O_HP], p[R.O_GAMMA], p[R.O_FULL], p[R.O_MSTATS]) == (R.FAM_FUSED8, 8, hp, g, full, ms)
        N, cus = c["N"], _cus()
        want_split = {1: (0, 0, N, -(-N // 16)), 0: (N, -(-N // 128), 0, 0), 2: (cus * 128, cus, 17, 2)}[tail]
        assert p[R.O_MAIN_ROWS:R.O_TAIL_GRID + 1] == want_split, (name, p)
        what = (name, "hot" if hot else "cold", "det" if det else "default")
        quanta = _quanta(c, ref) if det else None
        try:
            assert run.call() == PM_OK, what
            run.check(what, quanta)
            if det and c["stats"]:
                again = Fused8(dev, det, c, ref, pad=pad)
                assert again.call() == PM_OK, what
                for a, b in zip(_bits(*run.outputs()), _bits(*again.outputs())):
                    assert np.array_equal(a, b), (what, "two runs of the deterministic library differ")
        finally:
            if det:
                _forget_quanta()


# ------------------------------------------------------------------------------------------------------ modes and parts
@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
@pytest.mark.parametrize("name", ["main_hp8_g4_full_ms", "tail_hp6_g3_part_ms", "main_hp5_g3_part_e"])
def test_fused8_modes_and_parts(dev, name, det):
    """mode 1 (select only: logpj, lse and the statistics stay untouched), mode 2 (the candidates are an input, and not the
    ones a selection would return) and mode 3, each with part 0, 1 and 2: a part whose launch has no rows writes nothing.
    From both libraries; in the deterministic one a second run of a statistics call returns the same bits."""
    for mode in (1, 2, 3):
        stats = R.CASES[name]["stats"] and bool(mode & 2)
        c, ref = _case(name, mode == 3, given=(mode == 2))
        quanta = _quanta(c, ref) if det else None
        try:
            for part in (0, 1, 2):
                run = Fused8(dev, det, c, ref, mode=mode, part=part, stats=stats)
                what = (name, "mode", mode, "part", part, det)
                assert run.call() == PM_OK, what
                if run.lo == run.hi:
                    assert run.untouched(), (what, "a launch without rows wrote")
                    continue
                run.check(what, quanta)
                if det and stats:
                    again = Fused8(dev, det, c, ref, mode=mode, part=part, stats=stats)
                    assert again.call() == PM_OK, what
                    _same_bits(run.outputs(), again.outputs(), what)
        finally:
            if det:
                _forget_quanta()


def test_fused8_both_launches(dev):
    """N = cus 128 + 17: the main launch takes cus tiles, the TAIL launch 17 rows in two workgroups.  part 1 and part 2 write
    disjoint row ranges (the other range keeps the pattern: Fused8.check) whose union is bit for bit what part 0 writes;
    D_stats > D moves the sections behind Wp.  Deterministic library: a second run of every part returns the same bits, the
    statistics included."""
    name = "both_hp7_g3_part_ms"
    for det in (False, True):
        for hot in (True, False):
            c, ref = _case(name, hot)
            quanta = _quanta(c, ref) if det else None
            try:
                runs = []
                for part in (0, 1, 2):
                    run = Fused8(dev, det, c, ref, part=part, D_stats=c["D"] + 3)
                    what = (name, hot, det, "part", part)
                    assert run.plan[R.O_MAIN_ROWS] == _cus() * 128 and run.plan[R.O_TAIL_ROWS] == 17, run.plan
                    assert run.call() == PM_OK, what
                    run.check(what, quanta)
                    runs.append(run)
                    if det:
                        again = Fused8(dev, det, c, ref, part=part, D_stats=c["D"] + 3)
                        assert again.call() == PM_OK, what
                        _same_bits(run.outputs(), again.outputs(), what)
                m = runs[0].plan[R.O_MAIN_ROWS]
                for e0, e1, e2 in zip(*[(r.cand, r.el, r.es, r.ee) for r in runs]):
                    a, b1, b2 = _raw(e0), _raw(e1), _raw(e2)
                    rows = (lambda x, lo, hi: x[lo:hi] if x.shape[0] > 1 else x[:, lo:hi])
                    assert np.array_equal(rows(a, 0, m), rows(b1, 0, m)) and np.array_equal(rows(a, m, c["N"]), rows(b2, m, c["N"]))
            finally:
                if det:
                    _forget_quanta()


# ------------------------------------------------------------------------------------- lists, records, deferred statistics
def _apply(dev, det, run, cut, what, quanta):
    """pm_bsc_defer_apply_f64 on the outputs of a _defer run: the statistics become those of the datapoints with
    lse >= cut (reference: the in-pass statistics of those rows), the lists of the others are emptied, their dense rows
    zeroed; everything else keeps its bits."""
    c, ref = run.c, run.ref
    H, Hp, N, r = c["H"], c["Hp"], c["N"], c["rows"]
    lib = _lib_of(det)
    lse = run.es.host()[0]
    ecut = Emb(np.array([cut]), 1, dev)
    before = dict(idx=_raw(run.ei).copy(), val=_raw(run.ev).copy(), exp=_raw(run.ee).copy(), rec=_raw(run.er).copy(),
                  stats=run.est.host()[0].copy(), cand=_raw(run.cand).copy(), lse=_raw(run.es).copy())
    rc = lib.pm_bsc_defer_apply_f64(run.es.ptr, ecut.ptr, run.cand.ptr, run.er.ptr, run.ei.ptr, run.ev.ptr, run.ee.ptr, run.ee.ld,
                                    run.est.ptr, ctypes.byref(run.P), N, H, run.D_stats, Hp, _stream())
    torch.cuda.synchronize()
    assert rc == PM_OK, what
    keep = np.ones(N, dtype=bool) if cut < R.KEEP_ALL_BELOW else lse >= cut
    assert all(e.outside_untouched() for e in run.outputs()) and ecut.unchanged(), (what, "guards")
    for nm, e in (("val", run.ev), ("rec", run.er), ("cand", run.cand), ("lse", run.es)):
        assert np.array_equal(_raw(e), before[nm]), (what, nm, "an input of the apply pass changed")
    idx, exp = _raw(run.ei), _raw(run.ee)
    over = (before["idx"][:, 0].astype(np.int64) & 0xFFFF) == R.NZ_OVERFLOW
    assert np.array_equal(idx[keep], before["idx"][keep]) and np.array_equal(exp[keep], before["exp"][keep]), (what, "a kept row changed")
    assert ((idx[~keep].astype(np.int64) & 0xFFFF) == R.NZ_PAD).all(), (what, "the list of a dropped row was not emptied")
    assert (exp[~keep & over].view(np.float64) == 0).all(), (what, "the dense row of a dropped row was not zeroed")
    assert np.array_equal(exp[~keep & ~over], before["exp"][~keep & ~over]), (what, "a row that was never stored was written")
    # the kept rows' statistics: the reference of the distinct rows, weighted by how often each is kept
    keep_r = np.bincount(np.arange(N)[keep] % r, minlength=r)
    st = R.row_stats(ref["F"], ref["lse"], np.ones(r, dtype=bool), ref["E"], ref["cand"], c["SM"], H, c["ecoef"], mult=keep_r,
                     drop=R.dropped_onepass(ref["F64"]))
    # (sum lse is formed from the float64 lse the E-step stored: exactly representable addends)
    st["fs"] = np.asarray(lse[keep], dtype=LD).sum()
    want = R.pack_stats(st, H, run.D_stats, "fused8")
    _check_stats(run.est.host()[0], before["stats"], want, H, run.D_stats, quanta, N, what)
    return keep


@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
@pytest.mark.parametrize("name", R.LIST_CASES)
def test_fused8_lists_records_and_apply(dev, name, det):
    """_nz_f64: lists, overflowed rows (slot 0, the dense row, scalars[3]) against the reference, hot (every row overflows)
    and cold (rows with at most PM_BSC_NZ_MAX non-zeros and with more; among the cases a row with exactly 16 and rows with 17).  _defer_f64: nothing but scalars[3] is accumulated, the
    records hold the pair blocks and ecoef sum q e.  pm_bsc_defer_apply_f64 with the cut equal to one row's lse (kept), above
    every lse (none kept), and below log(2^-1075) (all kept).  records == NULL is _nz_f64 and nz_idx == NULL the plain entry,
    bit for bit in the deterministic library; there a second run of _nz_f64, of _defer_f64 with records and of
    pm_bsc_defer_apply_f64 on fresh outputs returns the same bits."""
    for hot in (True, False):
        c, ref = _case(name, hot)
        what = (name, "hot" if hot else "cold", "det" if det else "default")
        quanta = _quanta(c, ref) if det else None
        try:
            nz = Fused8(dev, det, c, ref, entry="nz")
            assert nz.call() == PM_OK, what
            nz.check(what + ("nz",), quanta)
            st_cnt = R.tile(c, R.row_stats(ref["F"], ref["lse"], np.ones(c["rows"], dtype=bool), ref["E"], ref["cand"], c["SM"], c["H"],
                                           c["ecoef"], drop=R.dropped_onepass(ref["F64"]))["nz_cnt"])
            assert (st_cnt > R.NZ_MAX).all() if hot else (st_cnt <= R.NZ_MAX).any(), what
            if det:
                nz2 = Fused8(dev, det, c, ref, entry="nz")
                assert nz2.call() == PM_OK, what
                _same_bits(nz.outputs(), nz2.outputs(), what + ("nz",))
                same = Fused8(dev, det, c, ref, entry="defer")
                assert same.call(records=None) == PM_OK, what
                for a, b in zip(_bits(*nz.outputs()), _bits(*same.outputs())):
                    assert np.array_equal(a, b), (what, "records == NULL differs from _nz_f64")
                plain, via = Fused8(dev, det, c, ref), Fused8(dev, det, c, ref, entry="nz")
                assert plain.call() == PM_OK and via.call(nzi=None, nzv=None) == PM_OK, what
                for a, b in zip(_bits(*plain.outputs()), _bits(*via.outputs())):
                    assert np.array_equal(a, b), (what, "nz_idx == NULL differs from the plain entry")
            lse_sorted = None
            for which in ("equal", "above", "all"):
                run = Fused8(dev, det, c, ref, entry="defer")
                assert run.call() == PM_OK, what
                run.check(what + ("defer",), quanta)
                lse = run.es.host()[0]
                lse_sorted = np.sort(lse)
                t = int(np.argsort(lse[:c["rows"]], kind="stable")[c["rows"] // 3])
                cut = {"equal": float(lse[t]), "above": max(float(lse_sorted[-1]) + 1.0, -700.0), "all": -800.0}[which]
                run2 = None
                if det:                  # a second _defer run on fresh outputs: the same bits, records included ...
                    run2 = Fused8(dev, det, c, ref, entry="defer")
                    assert run2.call() == PM_OK, what
                    _same_bits(run.outputs(), run2.outputs(), what + ("defer",))
                keep = _apply(dev, det, run, cut, what + ("apply", which), quanta)
                if det:                  # ... and after pm_bsc_defer_apply_f64 with the same cut, again
                    keep2 = _apply(dev, det, run2, cut, what + ("apply again", which), quanta)
                    assert np.array_equal(keep, keep2), what
                    _same_bits(run.outputs(), run2.outputs(), what + ("apply", which))
                # (cold, the evidences themselves lie below log(2^-1075): a cut taken from them keeps every datapoint)
                some_dropped = c["rows"] < 3 or cut < R.KEEP_ALL_BELOW or not keep.all()
                assert {"equal": keep[t] and some_dropped, "above": not keep.any(), "all": keep.all()}[which], what
        finally:
            if det:
                _forget_quanta()


# --------------------------------------------------------------------------------------------------------- return codes
@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
def test_fused8_return_codes_leave_the_outputs_untouched(dev, det):
    """Every PM_EINVAL / PM_ERANGE condition of the three fused8 entries and of pm_bsc_defer_apply_f64 once; nothing is
    launched (no output element moves).  N = 0 returns PM_OK and writes nothing.  From both libraries."""
    c, ref = _case("tail_hp6_g3_part_ms", True)
    H, D, K, S = c["H"], c["D"], c["K"], c["S"]
    if det:
        _quanta(c, ref)          # (the one launch below, whose outputs the refusals of the apply pass must leave alone)

    def call(entry="defer", **ov):
        run = Fused8(dev, det, c, ref, entry=entry)
        rc = run.call(**ov)
        assert run.untouched(), (entry, ov)
        return rc
    misaligned = Emb(c["Y"], D + 2, dev, off=1)
    assert misaligned.addr % 16 == 8
    for ov in (dict(Y=None), dict(Wt=None), dict(cand=None), dict(N=-1), dict(ldy=D - 2), dict(ldw=D - 2), dict(mode=0), dict(part=3),
               dict(part=-1), dict(P=None), dict(logpj=None), dict(ldl=K - 1), dict(gamma=0), dict(gamma=c["Hp"] + 1),
               dict(masks=None), dict(size_off=None), dict(expect=None), dict(lde=H - 1), dict(lse=None), dict(D_stats=0),
               dict(mode=1), dict(nzv=None), dict(stats=None), dict(Y=misaligned.ptr, ldy=D + 2), dict(ldy=D + 1),
               dict(ldw=D + 1), dict(wmu=ctypes.c_void_p(8))):
        assert call(**ov) == PM_EINVAL, ov
    assert call(entry="nz", stats=None, expect=None) == PM_EINVAL            # lists without statistics
    assert call(entry="defer", nzi=None, nzv=None) == PM_EINVAL              # records without lists
    bad_off = np.array([1, S], dtype=np.int32)
    assert call(size_off=bad_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == PM_EINVAL
    for ov in (dict(H=128, ldl=10 ** 6), dict(H=257, ldl=10 ** 6, lde=300), dict(D=D + 4, ldy=D + 4, ldw=D + 4), dict(Hp=4),
               dict(Hp=9), dict(S=S - 1), dict(mode=7), dict(gamma=4), dict(gamma=2)):
        assert call(**ov) == PM_ERANGE, ov
    assert call(N=0) == PM_OK and call(entry="plain", N=0) == PM_OK and call(entry="nz", N=0) == PM_OK

    run = Fused8(dev, det, c, ref, entry="defer")
    assert run.call() == PM_OK
    if det:
        _forget_quanta()
    lib = _lib_of(det)
    ecut = Emb(np.array([-800.0]), 1, dev)
    bits = _bits(*run.outputs())

    def apply(**ov):
        g = lambda k, d: ov.get(k, d)
        P = _params(c, **{k: v for k, v in ov.items() if k == "ecoef"})
        rc = lib.pm_bsc_defer_apply_f64(g("lse", run.es.ptr), g("cut", ecut.ptr), g("cand", run.cand.ptr), g("rec", run.er.ptr),
                                        g("nzi", run.ei.ptr), g("nzv", run.ev.ptr), g("expect", run.ee.ptr), g("lde", run.ee.ld),
                                        g("stats", run.est.ptr), g("P", ctypes.byref(P)), g("N", c["N"]), g("H", H), g("D", D),
                                        g("Hp", c["Hp"]), _stream())
        torch.cuda.synchronize()
        for a, b in zip(bits, _bits(*run.outputs())):
            assert np.array_equal(a, b), ("apply", ov)
        return rc
    for ov in (dict(lse=None), dict(cut=None), dict(cand=None), dict(rec=None), dict(nzi=None), dict(nzv=None), dict(expect=None),
               dict(stats=None), dict(P=None), dict(N=-1), dict(lde=H - 1)):
        assert apply(**ov) == PM_EINVAL, ov
    for ov in (dict(H=0, lde=300), dict(H=257, lde=300), dict(Hp=4), dict(Hp=9), dict(D=0), dict(ecoef=0.0)):
        assert apply(**ov) == PM_ERANGE, ov
    assert apply(N=0) == PM_OK


# ------------------------------------------------------------------------------------------------------ pm_bsc_select_f64
@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
@pytest.mark.parametrize("H", [sp["H"] for sp in R.CASES.values() if sp["entry"] == "select"])
def test_select(dev, H, det):
    """One H on each side of every VPL switch of bsc_select_kernel (confirmed with pm_bsc_plan), N = 1 and 5, |W_h|^2 read
    with stride 1 and, from the Gram diagonal in place, with stride H + 1.  The kernel divides by |W_h| and by |y|: |W_h| is a
    power of two and the quotients a / |W_h| are multiples of 1/4 below 2^10, so equal latents (equal rows of W) tie in any
    arithmetic and different ones stay apart by a relative gap of at least 2^-12 after the division by |y|."""
    lib = _lib_of(det)
    Hp = 6
    Wt = R.weights(H, 8, 11 + H)
    G = Wt @ Wt.T
    for N in (1, 5):
        Y = R.ints(N, 8, 3 + H + N, -6, 6)
        Y[:, 0] = np.where(Y[:, 0] == 0, 1.0, Y[:, 0])
        A, yn2 = Y @ Wt.T, (Y * Y).sum(axis=1)
        key = A / np.sqrt(np.diag(G))[None, :]
        assert (key * 4 == np.rint(key * 4)).all() and np.abs(key).max() < 2 ** 10
        want = R.select(A, np.diag(G), Hp, yn2=yn2)
        assert np.array_equal(want, R.rank_best_last(key, Hp))
        srt = np.sort(key, axis=1)
        assert (srt[:, -Hp] == srt[:, -Hp - 1]).any() or N == 1
        out = (ctypes.c_int32 * R.PLAN_LEN)()
        assert lib.pm_bsc_plan(R.SELECT, H, 0, Hp, 0, 0, 0, N, 0, out) == 0
        assert out[R.O_VPL] == (1 if H <= 64 else 2 if H <= 128 else 4 if H <= 256 else 8 if H <= 512 else 16)
        for stride in (1, H + 1):
            eA, eG, ey = Emb(A, H + 3, dev), Emb(G, H, dev), Emb(yn2, N, dev)
            ew = Emb(np.diag(G).copy(), H, dev)
            ec = _odd(np.zeros((N, Hp), dtype=np.int32), Hp, dev, fill=False)
            rc = lib.pm_bsc_select_f64(eA.ptr, eA.ld, ew.ptr if stride == 1 else eG.ptr, stride, ey.ptr, N, H, Hp, ec.ptr, _stream())
            torch.cuda.synchronize()
            assert rc == PM_OK and np.array_equal(ec.host(), want), (H, N, stride, ec.host().tolist(), want.tolist())
            assert ec.outside_untouched() and all(e.unchanged() for e in (eA, eG, ey, ew)), (H, N, stride)
    ec = _odd(np.zeros((1, Hp), dtype=np.int32), Hp, dev, fill=False)
    for ov, code in ((dict(lds=H - 1), PM_EINVAL), (dict(stride=0), PM_EINVAL), (dict(N=-1), PM_EINVAL), (dict(Hp=0), PM_EINVAL),
                     (dict(Hp=17), PM_ERANGE), (dict(H=1025, lds=2000), PM_ERANGE), (dict(N=0), PM_OK)):
        g = lambda k, d: ov.get(k, d)
        rc = lib.pm_bsc_select_f64(eA.ptr, g("lds", eA.ld), ew.ptr, g("stride", 1), ey.ptr, g("N", 1), g("H", H), g("Hp", Hp), ec.ptr,
                                   _stream())
        torch.cuda.synchronize()
        assert rc == code and ec.unchanged(), (H, ov, rc)


# ---------------------------------------------------------------------------------------------------- the sparse products
def _lists(N, H, seed):
    """Lists with integer values: empty, one entry, full (16 entries where H allows) and in between; valid slots lead, the
    latents of a list are distinct and ascending."""
    rng = np.random.RandomState(seed)
    idx = np.full((N, R.NZ_MAX), R.NZ_PAD, dtype=np.int64)
    val = np.zeros((N, R.NZ_MAX))
    for n in range(N):
        k = min(H, [0, 1, R.NZ_MAX, 5, R.NZ_MAX - 1][n % 5])
        idx[n, :k] = np.sort(rng.permutation(H)[:k])
        val[n, :k] = rng.randint(1, 8, size=k) * rng.choice([-1.0, 1.0], size=k)
    return idx, val


@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
@pytest.mark.parametrize("H,D,N", [(1, 1, 1), (255, 7, 257), (256, 8, 257), (256, 9, 1), (255, 65, 257)])
def test_sparse_products(dev, H, D, N, det):
    """pm_bsc_wp_sparse_f64, pm_bsc_expand_lists_gated_f64, pm_bsc_wp_sparse_expand_f64, pm_wp_sparse_f64 and
    pm_wp_sparse_t_f64 with integer values: the products are exact in any order, from both libraries.  Gate zero: the product
    is added, `expect` keeps its bits; gate non-zero: the product's output keeps its bits, the rows of complete lists are
    rebuilt, a row whose slot 0 reads PM_BSC_NZ_OVERFLOW keeps its dense values.  (An overflow-marked list never meets an open
    product: the marker and a non-zero gate are written together.)  Padded ldy, ldw, ldc and lde."""
    from prosper_amd import _lib
    from prosper_amd.em.camodels import _device
    lib = _lib_of(det)
    idx, val = _lists(N, H, 5 + H + D)
    Y = R.ints(N, D, 7 + N + D, -8, 8)
    Wp = R.wp_sparse(idx, val, Y, H).astype(np.float64)
    assert Wp.any() or N == 1
    if det:
        M8 = (ctypes.c_double * 8)(*([1.5 * 2.0 ** 31] * 8))            # quantum 2^-21: integers below 2^30 are exact addends
        _device._DET_QUANTA_SET.pop("wp_sparse", None)
        _lib.call("pm_det_set_quanta", _lib.DET_UNITS["wp_sparse"], M8, _stream(), det=True)
    marked = idx.copy()
    marked[::3, 0] = R.NZ_OVERFLOW                                    # every third list overflowed
    dense0 = R.ints(N, H, 9 + H, 1, 9)
    sc = R.stats_sections(H, D)["scalars"].start
    try:
        for gate in (0.0, 2.0):
            start = np.rint(_stats_start(R.stats_len(H, D)) * 8)
            start[sc + 3] = gate
            use = marked if gate else idx
            ei, ev = _odd(use.astype(np.uint16), R.NZ_MAX, dev), Emb(val, R.NZ_MAX, dev)
            eY = Emb(Y, D + 1, dev)
            want_stats = start.copy()
            if not gate:
                want_stats[:H * D] += Wp.reshape(-1)
            want_dense = R.expand_lists(use, val, H, dense0) if gate else dense0
            # pm_bsc_wp_sparse_f64
            est = _odd(start, len(start), dev)
            assert lib.pm_bsc_wp_sparse_f64(ei.ptr, ev.ptr, eY.ptr, eY.ld, est.ptr, N, H, D, _stream()) == PM_OK
            torch.cuda.synchronize()
            assert np.array_equal(est.host()[0], want_stats) and est.outside_untouched(), (H, D, N, gate, "wp_sparse")
            # pm_bsc_expand_lists_gated_f64
            ee, eg = Emb(dense0, H + 3, dev), Emb(np.array([gate]), 1, dev)
            assert lib.pm_bsc_expand_lists_gated_f64(ei.ptr, ev.ptr, ee.ptr, ee.ld, N, H, eg.ptr, _stream()) == PM_OK
            torch.cuda.synchronize()
            assert np.array_equal(ee.host(), want_dense) and ee.outside_untouched() and eg.unchanged(), (H, D, N, gate, "expand")
            assert gate or ee.unchanged()
            # pm_bsc_wp_sparse_expand_f64
            est, ee = _odd(start, len(start), dev), Emb(dense0, H + 1, dev)
            assert lib.pm_bsc_wp_sparse_expand_f64(ei.ptr, ev.ptr, eY.ptr, eY.ld, est.ptr, ee.ptr, ee.ld, N, H, D, _stream()) == PM_OK
            torch.cuda.synchronize()
            assert np.array_equal(est.host()[0], want_stats) and np.array_equal(ee.host(), want_dense), (H, D, N, gate, "both")
            assert est.outside_untouched() and ee.outside_untouched() and (gate or ee.unchanged())
            # pm_wp_sparse_f64: Wp and the gate given explicitly
            w0 = R.ints(H, D, 13, -3, 3)
            eW = Emb(w0, D + 2, dev)
            assert lib.pm_wp_sparse_f64(ei.ptr, ev.ptr, eY.ptr, eY.ld, eW.ptr, eW.ld, eg.ptr, N, H, D, _stream()) == PM_OK
            torch.cuda.synchronize()
            assert np.array_equal(eW.host(), w0 if gate else w0 + Wp) and eW.outside_untouched(), (H, D, N, gate, "pm_wp_sparse")
            assert all(e.unchanged() for e in (ei, ev, eY, eg)), (H, D, N, gate)
        # pm_wp_sparse_t_f64: the transposed output, no gate
        ei, ev, eY = _odd(idx.astype(np.uint16), R.NZ_MAX, dev), Emb(val, R.NZ_MAX, dev), Emb(Y, D + 1, dev)
        c0 = R.ints(D, H, 17, -3, 3)
        eC = Emb(c0, H + 1, dev)
        assert lib.pm_wp_sparse_t_f64(ei.ptr, ev.ptr, eY.ptr, eY.ld, eC.ptr, eC.ld, N, H, D, _stream()) == PM_OK
        torch.cuda.synchronize()
        assert np.array_equal(eC.host(), c0 + Wp.T) and eC.outside_untouched(), (H, D, N, "transposed")
        # return codes: nothing is written
        for call, code in ((lambda: lib.pm_wp_sparse_t_f64(ei.ptr, ev.ptr, eY.ptr, eY.ld, eC.ptr, H - 1, N, H, D, _stream()), PM_EINVAL),
                           (lambda: lib.pm_wp_sparse_t_f64(None, ev.ptr, eY.ptr, eY.ld, eC.ptr, eC.ld, N, H, D, _stream()), PM_EINVAL),
                           (lambda: lib.pm_wp_sparse_t_f64(ei.ptr, ev.ptr, eY.ptr, D - 1, eC.ptr, eC.ld, N, H, D, _stream()), PM_EINVAL),
                           (lambda: lib.pm_wp_sparse_t_f64(ei.ptr, ev.ptr, eY.ptr, eY.ld, eC.ptr, 300, N, 257, D, _stream()), PM_ERANGE),
                           (lambda: lib.pm_wp_sparse_t_f64(ei.ptr, ev.ptr, eY.ptr, eY.ld, eC.ptr, eC.ld, 0, H, D, _stream()), PM_OK),
                           (lambda: lib.pm_wp_sparse_f64(ei.ptr, ev.ptr, eY.ptr, eY.ld, eC.ptr, D, None, N, H, D, _stream()), PM_EINVAL),
                           (lambda: lib.pm_bsc_wp_sparse_f64(ei.ptr, ev.ptr, eY.ptr, eY.ld, None, N, H, D, _stream()), PM_EINVAL),
                           (lambda: lib.pm_bsc_expand_lists_gated_f64(ei.ptr, ev.ptr, eC.ptr, H - 1, N, H, eg.ptr, _stream()), PM_EINVAL),
                           (lambda: lib.pm_bsc_expand_lists_gated_f64(ei.ptr, ev.ptr, eC.ptr, H, N, H, None, _stream()), PM_EINVAL)):
            before = _raw(eC).copy()
            rc = call()
            torch.cuda.synchronize()
            assert rc == code and np.array_equal(_raw(eC), before) and eC.outside_untouched(), (H, D, N, rc, code)
    finally:
        if det:
            _device._DET_QUANTA_SET.pop("wp_sparse", None)


# ---------------------------------------------------------------------------------------------------------------------
# The other launchers: pm_bsc_estep_f64 / pm_bsc_mstep_rows_f64 (one wavefront per datapoint), pm_bsc_select_estep_f64,
# pm_bsc_mstep_rows16_f64 / _nz_f64 (sixteen lanes per datapoint) and pm_bsc_estep_fused_f64, one case per plan cell
# (bsc_kernels_reference.CASES, entry "wave", "select_estep", "rows16", "fused").  The row passes take the exact log-joints
# and the float64 lse as inputs; their reference uses the same lse and leaves out what the kernel documents (QCUT against
# the lse in bsc_mstep_rows16_kernel, nothing in bsc_mstep_rows_kernel).
# ---------------------------------------------------------------------------------------------------------------------
def _names(entry):
    return [n for n, s in R.CASES.items() if s["entry"] == entry]


def _score_inputs(dev, c, ref, pad, cand):
    """Operands of the entries that read the scores buffer; cand: the candidates as an input, or None for an output."""
    H, N, Hp = c["H"], c["N"], c["Hp"]
    ops = dict(A=Emb(c["A"], H + (3 if pad else 0), dev), G=Emb(c["G"], H, dev), yn2=Emb(c["yn2"], N, dev),
               masks=_odd(c["masks"], c["S"], dev), parents=_odd(c["parents"], c["S"], dev))
    if c["mu"] is not None:
        ops["wmu"], ops["ymu"] = Emb(c["wmu"], H, dev), Emb(c["ymu"], N, dev)
    if cand is not None:
        ops["cand"] = _odd(np.asarray(cand, dtype=np.int32), Hp, dev)
    return ops


def _so(c):
    return c["size_off"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _check_E(c, ref, got_F, got_lse, lanes, what):
    assert np.array_equal(got_F, ref["F64"]), (what, "logpj", np.argwhere(got_F != ref["F64"])[:5].tolist())
    err = np.abs(got_lse.astype(LD) - ref["lse"])
    bound = R.lse_bound(c["K"], lanes, ref["lse"].astype(np.float64))
    assert (err <= bound).all(), (what, "lse", float(err.max()), float(bound.min()))


def _cut_of(l64):
    """A cut that equals the lse of one datapoint bit for bit and lies above a third of the others; and that datapoint."""
    t = int(np.argsort(l64, kind="stable")[len(l64) // 3])
    return float(l64[t]), t


def _row_pass_reference(c, ref, l64, cut, drop_cut, conv, D_stats):
    keep = l64 >= cut
    drop = None if drop_cut is None else R.dropped(ref["F64"], l64, drop_cut)
    st = R.row_stats(ref["F"], l64, keep, ref["E"], ref["cand"], c["SM"], c["H"], c["ecoef"], drop=drop)
    over = int((keep & (st["nz_cnt"] > R.NZ_MAX)).sum())
    st["fs"] = np.asarray(l64[keep], dtype=LD).sum()
    return keep, st, over


def _check_rows(c, st, keep, exp, what, zeros=True):
    """zeros: the kernel has a documented cut-off, so an entry is zero exactly where the reference's is (without one a weight
    may underflow in float64 and not in longdouble)."""
    assert np.array_equal(exp[~keep], np.zeros_like(exp[~keep])), (what, "cut rows are not zero")
    assert row_rel(exp.astype(LD), st["expect"]) <= RTOL, (what, "expect", row_rel(exp.astype(LD), st["expect"]))
    assert not zeros or np.array_equal(exp == 0, np.asarray(st["expect"] == 0)), (what, "zeros of expect")


@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
@pytest.mark.parametrize("name", _names("wave"))
def test_wave_kernels(dev, name, det):
    """pm_bsc_estep_f64 and pm_bsc_mstep_rows_f64: (H, H', gamma) = (5, 3, 2), (12, 5, 3) with mu, (70, 6, 3), and S = 0; N = 1, 4
    and 5 straddle the four datapoints of a workgroup.  The row pass runs with lse_cut = -inf and with a cut that equals one
    row's lse (that row is kept, the rows below are zero rows).  Deterministic library: a second run of the row pass returns
    the same bits."""
    lib = _lib_of(det)
    for hot in (True, False):
        c, ref = _case(name, hot)
        H, Hp, S, N, D, K = c["H"], c["Hp"], c["S"], c["N"], c["D"], c["K"]
        what = (name, "hot" if hot else "cold", det)
        for which in (R.ESTEP, R.MSTEP_ROWS):
            rc, p = _plan(det, which, c, 0)
            assert rc == 0 and p[R.O_FAMILY] == R.WAVE and p[R.O_GRID] == -(-N // 4), (what, p)
        quanta = _quanta(c, ref) if det else None
        try:
            ops = _score_inputs(dev, c, ref, hot, ref["cand"])
            el, es = Emb(np.zeros((N, K)), K + (1 if hot else 0), dev, fill=False), Emb(np.zeros(N), N, dev, fill=False)
            P = _params(c)
            rc = lib.pm_bsc_estep_f64(ops["A"].ptr, ops["A"].ld, ops["G"].ptr, ops["yn2"].ptr, _p(ops, "wmu"), _p(ops, "ymu"),
                                      ops["cand"].ptr, ops["masks"].ptr if S else None, S, ctypes.byref(P), N, H, Hp, el.ptr, el.ld,
                                      es.ptr, _stream())
            torch.cuda.synchronize()
            assert rc == PM_OK, what
            _check_E(c, ref, el.host(), es.host()[0], 64, what)
            assert el.outside_untouched() and es.outside_untouched() and all(e.unchanged() for e in ops.values()), what
            l64 = ref["lse"].astype(np.float64)
            ptr, lst = R.pair_lists(c["SM"])
            for cut in (-np.inf, _cut_of(l64)[0]):
                keep, st, _ = _row_pass_reference(c, ref, l64, cut, None, "rows", D)
                eF, eL = Emb(ref["F64"], K + 2, dev), Emb(l64, N, dev)
                ep, eq = _odd(ptr, len(ptr), dev), _odd(lst, len(lst), dev)
                start = _stats_start(R.stats_len(H, D))

                def rows_once():
                    ee = Emb(np.zeros((N, H)), H + 1, dev, fill=False)
                    est = _odd(start, len(start), dev)
                    rc = lib.pm_bsc_mstep_rows_f64(eF.ptr, eF.ld, eL.ptr, ctypes.c_double(cut), ops["cand"].ptr,
                                                   ops["masks"].ptr if S else None, S, ep.ptr, eq.ptr if S else None, len(lst),
                                                   ctypes.byref(P), N, H, D, Hp, ee.ptr, ee.ld, est.ptr, _stream())
                    torch.cuda.synchronize()
                    assert rc == PM_OK, what
                    return ee, est
                ee, est = rows_once()
                if det:
                    _same_bits((ee, est), rows_once(), what + (cut,))
                _check_rows(c, st, keep, ee.host(), what + (cut,), zeros=False)
                _check_stats(est.host()[0], start, R.pack_stats(st, H, D, "rows"), H, D, quanta, N, what + (cut,))
                assert ee.outside_untouched() and est.outside_untouched(), what
                assert all(e.unchanged() for e in (eF, eL, ep, eq, ops["cand"], ops["masks"])), what
        finally:
            if det:
                _forget_quanta()


@pytest.mark.parametrize("name", _names("select_estep"))
def test_select_estep(dev, name):
    """pm_bsc_select_estep_f64 at every VPL boundary and one past it: mode 3, mode 1 (logpj and lse untouched), mode 2 with
    candidates that are not the selected ones, and under mode 1 the ranking bits 2 (smallest first), 3 (scores as they are)
    and 4 (|W_h|^2 - 2 a, without mu).  gamma = 1 (S = 0), 3 and 5; N in {1, 15, 16, 17, 65}; from both libraries."""
    spec = R.CASES[name]
    for det in (False, True):
        lib = _lib_of(det)
        for hot in (True, False):
            for mode in (3, 1, 2, 1 | 4, 1 | 8, 1 | 16):
                c, ref = _case(name, hot, given=(mode == 2))
                H, Hp, S, N, K = c["H"], c["Hp"], c["S"], c["N"], c["K"]
                what = (name, hot, det, "mode", mode)
                rc, p = _plan(det, R.SELECT_ESTEP, c, mode)
                assert rc == 0 and (p[R.O_FAMILY], p[R.O_VPL], p[R.O_MSTATS]) == spec["cell"] + ((mode >> 1) & 1,), (what, p)
                ops = _score_inputs(dev, c, ref, hot, None)
                plain = mode & ~3 == 0
                want = ref["cand"] if plain else R.select(c["A"], np.diag(c["G"]), Hp, mode)
                ec = _odd(np.asarray(ref["cand"], dtype=np.int32), Hp, dev, fill=(mode == 2))
                el, es = Emb(np.zeros((N, K)), K + (1 if hot else 0), dev, fill=False), Emb(np.zeros(N), N, dev, fill=False)
                P = _params(c)
                mu = plain and c["mu"] is not None
                rc = lib.pm_bsc_select_estep_f64(ops["A"].ptr, ops["A"].ld, ops["G"].ptr, ops["yn2"].ptr,
                                                 ops["wmu"].ptr if mu else None, ops["ymu"].ptr if mu else None,
                                                 ops["masks"].ptr if S else None, ops["parents"].ptr if S else None, _so(c), S,
                                                 c["gamma"], ctypes.byref(P), N, H, Hp, mode, ec.ptr, el.ptr, el.ld, es.ptr, _stream())
                torch.cuda.synchronize()
                assert rc == PM_OK, what
                if mode & 1:
                    assert np.array_equal(ec.host(), want), (what, "cand", np.argwhere(ec.host() != want)[:5].tolist())
                    assert ec.outside_untouched(), what
                else:
                    assert ec.unchanged(), what
                if mode & 2:
                    _check_E(c, ref, el.host(), es.host()[0], 16, what)
                    assert el.outside_untouched() and es.outside_untouched(), what
                else:
                    assert el.unchanged() and es.unchanged(), what
                assert all(e.unchanged() for e in ops.values()), what


def _check_row_lists(ei, ev, st, keep, what):
    """bsc_mstep_rows16_kernel's lists: the ascending non-zero latents of a kept row, the first PM_BSC_NZ_MAX of them, 0xFFFF
    behind them (a cut row: an empty list); slot 0 is not marked (the dense row is always stored)."""
    idx = _raw(ei).astype(np.int64) & 0xFFFF
    want_idx, _ = R.lists_of(st["expect"])
    assert np.array_equal(idx, want_idx), (what, "nz_idx", np.argwhere(idx != want_idx)[:5].tolist())
    raw_v = _raw(ev)
    filled = want_idx != R.NZ_PAD
    assert (raw_v[~filled] == ev.sent).all(), (what, "nz_val written behind a list")
    n_i, t_i = np.nonzero(filled)
    got_v, want_v = raw_v.view(np.float64)[n_i, t_i].astype(LD), st["expect"][n_i, want_idx[n_i, t_i]]
    assert (np.abs(got_v - want_v) <= RTOL * np.abs(st["expect"]).max(axis=1)[n_i]).all(), (what, "nz_val")


@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
@pytest.mark.parametrize("name", _names("rows16"))
def test_mstep_rows16(dev, name, det):
    """pm_bsc_mstep_rows16_f64 and _nz_f64 at every VPL boundary and one past it, plain and with lists (refused above
    H = 256: PM_ERANGE, nothing written), lse_cut = -inf and a cut that equals one row's lse (kept; the rows below it are zero
    rows with empty lists).  Hot, H = 16 has exactly PM_BSC_NZ_MAX non-zeros in every row and H = 17 one more (scalars[3]).
    Deterministic library: a second run of either entry returns the same bits (E[s], statistics, lists)."""
    lib = _lib_of(det)
    spec = R.CASES[name]
    for hot in (True, False):
        c, ref = _case(name, hot)
        H, Hp, S, N, D, K = c["H"], c["Hp"], c["S"], c["N"], c["D"], c["K"]
        l64 = ref["lse"].astype(np.float64)
        quanta = _quanta(c, ref) if det else None
        try:
            for lists in (False, True):
                rc, p = _plan(det, R.MSTEP_ROWS16, c, R.F_LISTS if lists else 0)
                assert (rc == PM_ERANGE) if (lists and H > 256) else \
                    (rc == 0 and (p[R.O_FAMILY], p[R.O_VPL], p[R.O_MSTATS]) == spec["cell"] + (int(lists),)), (name, rc, p)
                for cut in (-np.inf, _cut_of(l64)[0]):
                    what = (name, "hot" if hot else "cold", det, "lists" if lists else "plain", cut)
                    keep, st, over = _row_pass_reference(c, ref, l64, cut, R.QCUT, "rows", D)
                    eF, eL = Emb(ref["F64"], K + 2, dev), Emb(l64, N, dev)
                    ec, em = _odd(np.asarray(ref["cand"], dtype=np.int32), Hp, dev), _odd(c["masks"], S, dev)
                    start = _stats_start(R.stats_len(H, D))
                    P = _params(c)

                    def rows_once():
                        ee = Emb(np.zeros((N, H)), H + 1, dev, fill=False)
                        est = _odd(start, len(start), dev)
                        ei = _odd(np.zeros((N, R.NZ_MAX), dtype=np.uint16), R.NZ_MAX, dev, fill=False)
                        ev = Emb(np.zeros((N, R.NZ_MAX)), R.NZ_MAX, dev, fill=False)
                        args = (eF.ptr, eF.ld, eL.ptr, ctypes.c_double(cut), ec.ptr, em.ptr, S, ctypes.byref(P), N, H, D, Hp, ee.ptr,
                                ee.ld, est.ptr)
                        rc = lib.pm_bsc_mstep_rows16_nz_f64(*args, ei.ptr, ev.ptr, _stream()) if lists else \
                            lib.pm_bsc_mstep_rows16_f64(*args, _stream())
                        torch.cuda.synchronize()
                        return rc, ee, est, ei, ev
                    rc, ee, est, ei, ev = rows_once()
                    if det:
                        rc2, *second = rows_once()
                        assert rc2 == rc, what
                        _same_bits((ee, est, ei, ev), second, what)
                    assert all(e.unchanged() for e in (eF, eL, ec, em)), what
                    if lists and H > 256:
                        assert rc == PM_ERANGE and all(e.unchanged() for e in (ee, est, ei, ev)), (what, rc)
                        continue
                    assert rc == PM_OK, what
                    _check_rows(c, st, keep, ee.host(), what)
                    _check_stats(est.host()[0], start, R.pack_stats(st, H, D, "rows", overflow=over if lists else 0), H, D,
                                 quanta, N, what)
                    assert ee.outside_untouched() and est.outside_untouched(), what
                    if lists:
                        _check_row_lists(ei, ev, st, keep, what)
                        assert ei.outside_untouched() and ev.outside_untouched(), what
                        if hot and H in (16, 17) and cut == -np.inf:
                            assert (st["nz_cnt"] == H).all() and over == (N if H == 17 else 0), (what, st["nz_cnt"])
                    else:
                        assert ei.unchanged() and ev.unchanged(), what
        finally:
            if det:
                _forget_quanta()


@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
@pytest.mark.parametrize("name", _names("fused"))
def test_fused(dev, name, det):
    """pm_bsc_estep_fused_f64: NJ = 8 (H = 16, 128) and 16 (H = 129, 256), FULL and not, with and without statistics; N in
    {1, 63, 64, 65, 129}; D = 8, one K-step short of the four-stage ring, the ring, one more; D_stats > D.  The statistics
    leave the multi-cause diagonal in the Wq block and do not write qdiag.  fused_h128_ms also runs mode 1 and mode 2.
    Deterministic library: a second run of a statistics call returns the same bits."""
    lib = _lib_of(det)
    spec = R.CASES[name]
    modes = (3, 1, 2) if name == "fused_h128_ms" else (3,)
    for hot in (True, False):
        for mode in modes:
            c, ref = _case(name, hot, given=(mode == 2))
            H, Hp, S, N, D, K = c["H"], c["Hp"], c["S"], c["N"], c["D"], c["K"]
            stats = c["stats"] and bool(mode & 2)
            Ds = D + 5
            what = (name, "hot" if hot else "cold", det, "mode", mode)
            rc, p = _plan(det, R.FUSED, c, mode | (R.F_STATS if stats else 0))
            assert rc == 0 and (p[R.O_FAMILY], p[R.O_NJ], p[R.O_FULL], p[R.O_MSTATS]) == spec["cell"][:3] + (int(stats),), (what, p)
            assert p[R.O_GRID] == -(-N // 64)
            quanta = _quanta(c, ref) if det else None
            try:
                ops = _inputs(dev, c, hot)
                start = _stats_start(R.stats_len(H, Ds))
                P = _params(c)

                def fused_once():
                    ec = _odd(np.asarray(ref["cand"], dtype=np.int32), Hp, dev, fill=(mode == 2))
                    el, es = Emb(np.zeros((N, K)), K + 1, dev, fill=False), Emb(np.zeros(N), N, dev, fill=False)
                    ee = Emb(np.zeros((N, H)), H + (1 if hot else 0), dev, fill=False)
                    est = _odd(start, len(start), dev)
                    rc = lib.pm_bsc_estep_fused_f64(ops["Y"].ptr, ops["Y"].ld, ops["Wt"].ptr, ops["Wt"].ld, ops["G"].ptr,
                                                    ops["yn2"].ptr, _p(ops, "wmu"), _p(ops, "ymu"), ops["masks"].ptr,
                                                    ops["parents"].ptr, _so(c), S, c["gamma"], ctypes.byref(P), N, D, H, Hp, mode,
                                                    ec.ptr, el.ptr, el.ld, es.ptr, ee.ptr if stats else None, ee.ld,
                                                    est.ptr if stats else None, Ds, _stream())
                    torch.cuda.synchronize()
                    assert rc == PM_OK, what
                    return ec, el, es, ee, est
                ec, el, es, ee, est = fused_once()
                if det and stats:
                    _same_bits((ec, el, es, ee, est), fused_once(), what)
                assert all(e.unchanged() for e in ops.values()), what
                if mode & 1:
                    assert np.array_equal(ec.host(), ref["cand"]) and ec.outside_untouched(), (what, "cand")
                else:
                    assert ec.unchanged(), what
                if not mode & 2:
                    assert all(e.unchanged() for e in (el, es, ee, est)), what
                    continue
                _check_E(c, ref, el.host(), es.host()[0], 16, what)
                assert el.outside_untouched() and es.outside_untouched(), what
                if not stats:
                    assert ee.unchanged() and est.unchanged(), what
                    continue
                st = R.row_stats(ref["F"], ref["lse"], np.ones(N, dtype=bool), ref["E"], ref["cand"], c["SM"], H, c["ecoef"],
                                 drop=R.dropped_onepass(ref["F64"]))
                _check_rows(c, st, np.ones(N, dtype=bool), ee.host(), what)
                _check_stats(est.host()[0], start, R.pack_stats(st, H, Ds, "fused"), H, Ds, quanta, N, what)
                assert ee.outside_untouched() and est.outside_untouched(), what
            finally:
                if det:
                    _forget_quanta()


@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
def test_other_return_codes(dev, det):
    """PM_EINVAL / PM_ERANGE branches of pm_bsc_estep_f64, pm_bsc_mstep_rows_f64, pm_bsc_select_estep_f64,
    pm_bsc_mstep_rows16_nz_f64 and pm_bsc_estep_fused_f64; no output element moves.  N = 0 returns PM_OK.  From both libraries."""
    lib = _lib_of(det)
    c, ref = _case("r16_h33", True)
    H, Hp, S, N, D, K = c["H"], c["Hp"], c["S"], c["N"], c["D"], c["K"]
    ops, yw = _score_inputs(dev, c, ref, True, ref["cand"]), _inputs(dev, c, True)
    l64 = ref["lse"].astype(np.float64)
    eF, eL = Emb(ref["F64"], K + 2, dev), Emb(l64, N, dev)
    ptr, lst = R.pair_lists(c["SM"])
    ep, eq = _odd(ptr, len(ptr), dev), _odd(lst, len(lst), dev)
    outs = dict(el=Emb(np.zeros((N, K)), K + 1, dev, fill=False), es=Emb(np.zeros(N), N, dev, fill=False),
                ee=Emb(np.zeros((N, H)), H + 1, dev, fill=False), est=Emb(_stats_start(R.stats_len(H, D)), R.stats_len(H, D), dev),
                ei=_odd(np.zeros((N, 16), dtype=np.uint16), 16, dev, fill=False), ev=Emb(np.zeros((N, 16)), 16, dev, fill=False),
                ec=_odd(np.zeros((N, Hp), dtype=np.int32), Hp, dev, fill=False))
    P = _params(c)

    def call(entry, **ov):
        g = lambda k, d: ov.get(k, d)
        Pp = g("P", ctypes.byref(P))
        h, hp, n, s = g("H", H), g("Hp", Hp), g("N", N), g("S", S)
        if entry == "estep":
            rc = lib.pm_bsc_estep_f64(g("A", ops["A"].ptr), g("lds", ops["A"].ld), ops["G"].ptr, ops["yn2"].ptr, g("wmu", None), None,
                                      ops["cand"].ptr, g("masks", ops["masks"].ptr), s, Pp, n, h, hp, g("logpj", outs["el"].ptr),
                                      g("ldl", K + 1), outs["es"].ptr, _stream())
        elif entry == "rows":
            rc = lib.pm_bsc_mstep_rows_f64(g("F", eF.ptr), g("ldl", eF.ld), eL.ptr, ctypes.c_double(-np.inf), ops["cand"].ptr,
                                           g("masks", ops["masks"].ptr), s, g("pp", ep.ptr), eq.ptr, g("plen", len(lst)), Pp, n, h,
                                           g("D", D), hp, outs["ee"].ptr, g("lde", H + 1), g("stats", outs["est"].ptr), _stream())
        elif entry == "select_estep":
            rc = lib.pm_bsc_select_estep_f64(g("A", ops["A"].ptr), g("lds", ops["A"].ld), ops["G"].ptr, ops["yn2"].ptr, g("wmu", None),
                                             None, g("masks", ops["masks"].ptr), ops["parents"].ptr, _so(c), s, g("gamma", c["gamma"]),
                                             Pp, n, h, hp, g("mode", 3), outs["ec"].ptr, g("logpj", outs["el"].ptr), g("ldl", K + 1),
                                             outs["es"].ptr, _stream())
        elif entry == "rows16":
            rc = lib.pm_bsc_mstep_rows16_nz_f64(g("F", eF.ptr), g("ldl", eF.ld), eL.ptr, ctypes.c_double(-np.inf), ops["cand"].ptr,
                                                g("masks", ops["masks"].ptr), s, Pp, n, h, g("D", D), hp, outs["ee"].ptr,
                                                g("lde", H + 1), g("stats", outs["est"].ptr), g("nzi", outs["ei"].ptr),
                                                g("nzv", outs["ev"].ptr), _stream())
        else:
            rc = lib.pm_bsc_estep_fused_f64(g("Y", yw["Y"].ptr), g("ldy", yw["Y"].ld), yw["Wt"].ptr, g("ldw", yw["Wt"].ld), ops["G"].ptr,
                                            ops["yn2"].ptr, g("wmu", None), None, g("masks", ops["masks"].ptr), ops["parents"].ptr,
                                            _so(c), s, g("gamma", c["gamma"]), Pp, n, g("D", D), h, hp, g("mode", 3), outs["ec"].ptr,
                                            g("logpj", outs["el"].ptr), g("ldl", K + 1), g("lse", outs["es"].ptr),
                                            g("expect", outs["ee"].ptr), g("lde", H + 1), g("stats", outs["est"].ptr), g("Ds", D),
                                            _stream())
        torch.cuda.synchronize()
        assert all(e.unchanged() for e in outs.values()), (entry, ov)
        return rc
    for entry in ("estep", "rows", "select_estep", "rows16", "fused"):
        assert call(entry, N=-1) == PM_EINVAL and call(entry, Hp=0) == PM_EINVAL and call(entry, ldl=K - 1) == PM_EINVAL, entry
        assert call(entry, masks=None) == PM_EINVAL and call(entry, S=-1) == PM_EINVAL, entry
        assert call(entry, Hp=17) == PM_ERANGE and call(entry, N=0) == PM_OK, entry
        assert call(entry, H=4, lds=4) == PM_ERANGE, entry                               # Hprime > H
    for entry in ("estep", "rows", "select_estep", "rows16"):
        assert call(entry, P=None) == PM_EINVAL, entry
    for entry in ("estep", "select_estep", "fused"):
        assert call(entry, wmu=ctypes.c_void_p(8)) == PM_EINVAL and call(entry, logpj=None) == PM_EINVAL, entry
    for entry in ("estep", "select_estep"):
        assert call(entry, A=None) == PM_EINVAL and call(entry, lds=H - 1) == PM_EINVAL, entry
    for entry in ("rows", "rows16"):
        assert call(entry, F=None) == PM_EINVAL and call(entry, lde=H - 1) == PM_EINVAL and call(entry, D=0) == PM_EINVAL, entry
        assert call(entry, stats=None) == PM_EINVAL, entry
    assert call("estep", H=1025, lds=1025, ldl=2000) == PM_ERANGE and call("estep", S=65536, ldl=10 ** 6) == PM_ERANGE
    assert call("rows", pp=None) == PM_EINVAL and call("rows", plen=-1) == PM_EINVAL
    assert call("rows", S=65536, ldl=10 ** 6) == PM_ERANGE
    assert call("select_estep", mode=0) == PM_EINVAL and call("select_estep", gamma=0) == PM_EINVAL
    assert call("select_estep", gamma=Hp + 1) == PM_EINVAL and call("select_estep", H=513, lds=513, ldl=1000) == PM_ERANGE
    assert call("select_estep", S=4097, ldl=10 ** 6) == PM_ERANGE
    assert call("rows16", nzv=None) == PM_EINVAL and call("rows16", H=257, ldl=1000, lde=300) == PM_ERANGE
    assert call("rows16", H=513, ldl=1000, lde=600) == PM_ERANGE
    assert call("fused", Y=None) == PM_EINVAL and call("fused", ldy=D - 2) == PM_EINVAL and call("fused", mode=0) == PM_EINVAL
    assert call("fused", gamma=0) == PM_EINVAL and call("fused", expect=None) == PM_EINVAL and call("fused", lse=None) == PM_EINVAL
    assert call("fused", Ds=0) == PM_EINVAL and call("fused", mode=1) == PM_EINVAL and call("fused", ldy=yw["Y"].ld + 1) == PM_EINVAL
    assert call("fused", H=257, ldl=1000, lde=300) == PM_ERANGE and call("fused", D=D + 4, ldy=D + 4, ldw=D + 4) == PM_ERANGE
    assert call("fused", mode=7) == PM_ERANGE and call("fused", Hp=9, gamma=3, ldl=1000) == PM_ERANGE     # stats with H' > 8
