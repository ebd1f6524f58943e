"""The GSC kernels (gsc_kernels.hip) through the C ABI -- pm_gsc_estep_f64, pm_gsc_estep_lpj_f64, pm_gsc_estep_lpj_blocks_f64,
pm_gsc_estep_lists_f64, pm_gsc_list_pairs_f64, pm_gsc_pack_stats_f64, pm_gsc_component_scores_f64 -- on padded, guarded operands,
one smallest shape per dispatch cell (confirmed with pm_gsc_plan inside the test, with the device's CU count: a case that
lands in another instantiation fails), against the plain NumPy reference tests/gsc_kernels_reference.py, from both libraries.

Harness: ``Emb`` of tests/test_eval_kernels_gpu.py (16 guard rows before and after, padding columns, a quiet-NaN payload /
0xDEADBEEF pattern; 0xA5A5 for the uint16 state masks and list indices, carried as int16).  `cand` and `state_masks` start at
odd element offsets; scores, xpt_s / xpt_sz, the log-joints and the blocks have padded leading dimensions.  After every call
the results are compared with the reference, every guard and padding element of every output still holds the pattern, every
input is bit-unchanged, and the scratch tail of `stats` (seven per-XCD copies of 2 H^2) is all zeros again.  `stats` starts
from position-dependent multiples of 1/8, so that "accumulates into" is tested; entries no datapoint contributes to (the
lower triangle and the diagonal of U_ss, pairs that share no state, entries below thr_p) come back bit-unchanged.

Exact (equality): `cand`, the list indices and terminators, *dense_count and the set of dense rows, pm_gsc_list_pairs_f64 on
integer values, pm_gsc_component_scores_f64 on the exact inputs of the selection cases, pm_gsc_pack_stats_f64 given the raw
statistics it read (one float64 addition per diagonal entry).

Bounded, against the longdouble reference (u = 2^-53, RTOL = 1e-11 of tests/test_eval_kernels_gpu.py, FLOOR = 1e-290):
  logpj      |err| <= B_nk = RTOL max_k |lp_nk| + 4 canc_nk + FLOOR; canc_nk is the reference's cancellation term of the state:
             |r|^2 = yn + sum mu (G mu - 2 a) and quad = b^T Lambda^-1 b are sums of terms far larger than their result when
             y ~ W mu, so their rounding is u (|yn| + sum |mu| (|G mu| + 2 |a|)) / s2 + u sum |b||Lambda^-1||b| / s2^2
             whatever the result is (tests/mca_kernels_reference.sigma_cancellation has the same form).
  weights and everything normalised (xpt_s, xpt_sz, blocks): a weight is exp(beta lp); an error d in lp is a RELATIVE error
             beta d in the weight.  With B_n = max_k B_nk every weight of the row is off by at most beta B_n relative, so a
             sum of weighted terms is off by beta B_n of the sum of their magnitudes, and a normalised one -- numerator and
             Z both move -- by 2 beta B_n.  Bound: (RTOL + 2 beta B_n) x the row's largest sum of magnitudes (for xpt_sz the
             reference also carries sum |w kappa|), + FLOOR.  B_n contains RTOL |beta lp|_max: the widening the argument of
             exp asks for.  A state whose beta lp lies within B_n of log(tiny) may be clamped on one side and not on the
             other: both values are tiny to 1e-11, so no case is excluded for that.
  statistics  section-relative (U_ss, U_zz, cs, csz, dzz; packed: five sections) to the section's largest accumulated
             magnitude (start + sum over datapoints of |contribution|), with the largest row bound above, widened by N u
             because the atomics land in any order; deterministic library: quanta for PM_DET_GSC installed as
             test_mca_kernels_gpu._install_quanta does for `mca` (A = 4 (max |start + result| + N max |addend|), bound 2^k >= A,
             quantum 2^(k - 51)), widened by (N + 1) quantum / 2.
No case is excluded from any comparison.

Worst observed error as a fraction of its bound (MI355X, both libraries, 278 tests pass on the unchanged source in 21 s; the
module's autouse fixture prints the table with -s):
                          HOT default   HOT deterministic   COLD default   COLD deterministic
  logpj                   0.012         0.012               6.3e-5         6.3e-5
  xpt_s / xpt_sz          1.7e-4        1.7e-4              1.8e-5         1.8e-5
  blocks, list values     9.4e-5        9.4e-5              1.4e-5         1.4e-5
  raw statistics          0.001         0.21                4e-6           0.008
  packed statistics       3e-5          0.008               3e-6           4e-6
The bounds are the ones derived above, not fitted: the kernel sits one to five orders of magnitude inside them, the
deterministic library's quantised statistics a factor five.

Mutants of gsc_kernels.hip (values and predicates only: none changes an address, a trip count or the number of selected
latents), each run once against this module, default library, MI355X (140 tests pass on the unchanged source):
   1 final `flush_pairs(false)` removed            112 fail: test_estep (54: all but the six cells without a multi-cause state),
                                                   test_estep_lpj (30), test_estep_lpj_blocks (11), test_lists (4),
                                                   test_pair_threshold (5), test_second_trip (4), test_state_trip_edges (4)
   2 `pend = live` -> `true`                       112: the same tests (N % 16 != 0: the dead lanes send row N - 1 again)
   3 `k > i` -> `k >= i` in the U_ss send          112: the same tests (the diagonal of U_ss is "an entry no datapoint
                                                   contributes to")
   4 `-708.3964185322641` -> `-708.0` in gsc_weight (both places: the window's states become `tiny`)
                                                   120: every COLD run -- test_estep (60), test_estep_lpj (30), _blocks (11),
                                                   test_lists (4), test_pair_threshold (5), test_second_trip (4),
                                                   test_state_trip_edges (6)
   5 the libm window removed                       120: the same tests
   6 `0x3FF - h` -> `h` for negative keys          11: test_selection at every shape but H = H' = 1
   7 `nsig <= PM_BSC_NZ_MAX` -> `<`                5: test_lists (4), test_second_trip[t_v8_g2]
   8 `vs > thr` dropped from `sig`                 5: test_lists (4), test_second_trip[t_v8_g2]
   9 gsc_colsum_kernel launched under `lacc` too   65: every LACC / LIST run -- test_estep (30), test_estep_lpj (20: the
                                                   statistics form of the same operands), test_lists (4), test_pair_threshold
                                                   (3), test_second_trip (2), test_state_trip_edges (6)
  10 `kind ? vz : nz_vs` swapped in list pairs     4: test_list_pairs at every H
  11 `thr_p` read when `inv_s2_host != 0`          110: every run with sigma_sq > 0 and H > 2 (the ninth table row is not handed
                                                   in there: the kernel reads the guard pattern)
  12 `nf_prev` kept from a workgroup's FIRST trip  4: test_second_trip, all four forms, and nothing else.  (It first SURVIVED: with
                                                   rows repeating at period 64 and 16 x the grid cap a multiple of 64, a workgroup
                                                   met the same rows on every trip.  The rows are shifted by five per trip now.)
No mutant is equivalent.  (Changing only the clamp line of gsc_weight to -708.0 IS equivalent -- the window's arguments
return before it -- which is why mutant 4 changes both places.)
"""
import ctypes
import functools

import numpy as np
import pytest

import gsc_kernels_reference as R
from test_eval_kernels_gpu import GUARD_ROWS, LAYOUTS, RTOL, Emb as _Emb, _ld, _stream, dev, row_rel  # noqa: F401

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT_U16 = 0xA5A5 - 0x10000
PM_OK, PM_EINVAL, PM_ERANGE = 0, -1, -2
LD = np.longdouble
FLOOR = 1e-290
U = 2.0 ** -53
STAT_NAMES = [n for n in R.CASES if R.CASES[n][6][2] in (R.PLAIN, R.LACC)]
LPJ_NAMES = [n for n in R.CASES if R.CASES[n][6][2] == R.LPJ]
LIST_NAMES = [n for n in R.CASES if R.CASES[n][6][2] == R.LIST]
SMALL_N = {"a_v1_g3": (1, 16), "p_v2_g2": (1, 16), "l_v1_g3": (1, 16), "t_v8_g2": (1, 16)}     # one case per form
ALL_LAYOUT_CASE = "a_v2_g3"
WORST = {}                          # (entry, quantity, HOT / COLD, library) -> (error / bound, error, bound)


class Emb(_Emb):
    """... and uint16 operands (state masks, list indices), carried as int16."""
    _TYPES = dict(_Emb._TYPES)
    _TYPES[np.dtype(np.int16)] = (torch.int16, SENT_U16)


def _odd(array, ld, dev, fill=True):
    """An operand that starts at an odd element offset of its buffer."""
    e = Emb(array, ld, dev, off=1 if (GUARD_ROWS * ld) % 2 == 0 else 2, fill=fill)
    assert e.start % 2 == 1
    return e


def _lib_of(det):
    from prosper_amd import _lib
    return _lib.load(det)


@functools.lru_cache(maxsize=None)
def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _plan(det, which, H, Hp, S, gamma, D, flags, N):
    out = (ctypes.c_int32 * R.PLAN_LEN)(*([-7] * R.PLAN_LEN))
    rc = _lib_of(det).pm_gsc_plan(which, H, Hp, S, gamma, D, flags, N, _cus(), out)
    return rc, tuple(out)


def _assert_cell(det, c, flags=None, N=None):
    """The case lands in the instantiation it is meant for; returns the plan."""
    flags = c["flags"] if flags is None else flags
    rc, p = _plan(det, R.ESTEP, c["H"], c["Hp"], c["S"], c["gamma"], 0, flags, c["N"] if N is None else N)
    want = c["cell"]
    if flags != c["flags"]:          # the same operands through another entry point: VPL and GMAX stay, the form follows
        form = R.LPJ if flags & R.F_LPJ else R.LIST if flags & R.F_LISTS else None
        assert rc == PM_OK and p[:2] == want[:2] and (form is None or p[2] == form), (c["name"], flags, rc, p)
    else:
        assert rc == PM_OK and p[:3] == want, (c["name"], rc, p)
    return p


@functools.lru_cache(maxsize=None)
def _case(name, hot, N=None):
    """Operands and reference of a case, computed once and shared by every test (and both libraries)."""
    c = R.make_case(name, hot, N)
    cand = R.select(c)
    return c, cand, R.estep(c, cand)


def _note(entry, what, hot, det, err, bound):
    key = (entry, what, "HOT" if hot else "COLD", "det" if det else "default")
    ratio = float(err) / float(bound) if bound > 0 else 0.0
    if ratio > WORST.get(key, (-1.0, 0.0, 0.0))[0]:
        WORST[key] = (ratio, float(err), float(bound))


def _row_bounds(c, e):
    """(B_nk, rel_n): the log-joint bound of every state and the relative bound of a row's weighted sums (module docstring)."""
    B = RTOL * np.abs(e["lp"]).max(axis=1)[:, None] + 4 * e["canc"] + FLOOR
    rel = RTOL + 2 * LD(c["beta"]) * B.max(axis=1)
    return B, rel


def _close_rows(got, want, scale, rel, entry, what, hot, det, tag):
    got, want = np.asarray(got).astype(LD), np.asarray(want, dtype=LD)
    err = np.abs(got - want).max(axis=1)
    bound = rel * scale + FLOOR
    i = int(np.argmax(err / bound))
    _note(entry, what, hot, det, err[i], bound[i])
    assert (err <= bound).all(), (tag, what, "row", i, float(err[i]), float(bound[i]))


def _stats_start(H):
    """Non-zero, position-dependent multiples of 1/8 in the documented part; the scratch tail starts (and must end) at zero."""
    s = np.zeros(R.stats_len(H))
    base = R.stats_base(H)
    s[:base] = (1 + (np.arange(base) * 5) % 8) / 8.0
    return s


def _abs_of(e):
    """The reference with every contribution replaced by its magnitude: the scale of a statistic."""
    return dict(e, xpt_sz=e["xsz_abs"], pair_zz=np.abs(e["pair_zz"]), pair_ss=np.abs(e["pair_ss"]))


def _install_quanta(total_abs, addend_max, N):
    """Quanta of unit `gsc` in the deterministic library (module docstring); returns the quantum."""
    from prosper_amd import _lib
    from prosper_amd.em.camodels import _device
    A = 4.0 * (float(np.abs(total_abs).max()) + N * max(1.0, float(addend_max)))
    k = int(np.ceil(np.log2(A)))
    M8 = (ctypes.c_double * 8)(*([1.5 * 2.0 ** (k + 1)] * 8))
    _device._DET_QUANTA_SET.pop("gsc", None)
    _lib.call("pm_det_set_quanta", _lib.DET_UNITS["gsc"], M8, _stream(), det=True)
    torch.cuda.synchronize()
    return 2.0 ** (k - 51)


def _addend_max(e):
    return max(float(e["xsz_abs"].max(initial=0)), float(np.abs(e["pair_zz"]).max(initial=0)), float(e["single_zz"].max(initial=0)),
               1.0)


class Run:
    """One launch of an E-step entry point on guarded operands."""

    def __init__(self, dev, det, c, cand, entry="estep", layout="odd", select=True, sigma0=False, tables=None, scores=None,
                 ynorm2=None, N=None, null_masks=False, stats_start=None):
        H, Hp, S = c["H"], c["Hp"], c["S"]
        scores = c["scores"] if scores is None else scores
        yn = c["ynorm2"] if ynorm2 is None else ynorm2
        N = scores.shape[0] if N is None else N
        self.c, self.N, self.entry, self.det, self.select = c, N, entry, det, select
        t = c["tables"] if tables is None else tables
        # sigma_sq > 0 and no lists: the ninth row is not an operand, the guard pattern (NaN) follows the eighth
        tflat = t.reshape(-1) if (sigma0 or entry == "lists") else t[:8].reshape(-1)
        self.ops = dict(scores=Emb(scores, _ld(H, layout, 0), dev), gram=Emb(c["gram"], H, dev), psi=Emb(c["psi_sq"], H, dev),
                        yn=Emb(yn, len(yn), dev), tables=Emb(tflat, len(tflat), dev))
        if S and not null_masks:
            self.ops["masks"] = _odd(c["masks"].view(np.int16), S, dev)
        self.cand = _odd(np.ascontiguousarray(cand, dtype=np.int32), Hp, dev, fill=not select)
        ldx = _ld(H, layout, 1)
        self.xs = Emb(np.zeros((N, H)), ldx, dev, fill=False)
        self.xsz = Emb(np.zeros((N, H)), ldx, dev, fill=False)
        self.start = _stats_start(H) if stats_start is None else stats_start
        self.stats = Emb(self.start.reshape(H, -1), len(self.start) // H, dev)
        self.outs = [self.xs, self.xsz, self.stats] + ([self.cand] if select else [])
        K, B = 1 + H + S, 2 * Hp * Hp + 2 * Hp + 1
        self.logpj = self.blocks = self.nz_idx = None
        if entry in ("lpj", "blocks"):
            self.logpj = Emb(np.zeros((N, K)), _ld(K, layout, 2), dev, fill=False)
            self.outs.append(self.logpj)
        if entry == "blocks":
            self.blocks = Emb(np.zeros((N, B)), _ld(B, layout, 0), dev, fill=False)
            self.outs.append(self.blocks)
        if entry == "lists":
            self.nz_idx = Emb(np.zeros((N, R.NZ_MAX), dtype=np.int16), R.NZ_MAX, dev, fill=False)
            self.nz_val = Emb(np.zeros((2 * N, R.NZ_MAX)), R.NZ_MAX, dev, fill=False)
            self.dense_rows = Emb(np.zeros(N, dtype=np.int32), N, dev, fill=False)
            self.dense_count = Emb(np.zeros(1, dtype=np.int32), 1, dev)
            self.outs += [self.nz_idx, self.nz_val, self.dense_rows, self.dense_count]
        self.sigma_arg = 0.0 if sigma0 else c["sigma_sq"]

    def launch(self, **over):
        c, o = self.c, self.ops
        a = dict(scores=o["scores"].ptr, lds=o["scores"].ld, gram=o["gram"].ptr, psi=o["psi"].ptr, yn=o["yn"].ptr,
                 tables=o["tables"].ptr, masks=o["masks"].ptr if "masks" in o else None, S=c["S"], gamma=c["gamma"],
                 beta=c["beta"], sigma_sq=self.sigma_arg, N=self.N, H=c["H"], Hp=c["Hp"], select=int(self.select),
                 cand=self.cand.ptr, xs=self.xs.ptr, xsz=self.xsz.ptr, ldx=self.xs.ld, stats=self.stats.ptr)
        a.update(over)
        head = (a["scores"], a["lds"], a["gram"], a["psi"], a["yn"], a["tables"], a["masks"], a["S"], a["gamma"],
                ctypes.c_double(a["beta"]), ctypes.c_double(a["sigma_sq"]), a["N"], a["H"], a["Hp"], a["select"], a["cand"], a["xs"],
                a["xsz"], a["ldx"], a["stats"])
        lib = _lib_of(self.det)
        if self.entry == "estep":
            rc = lib.pm_gsc_estep_f64(*head, _stream())
        elif self.entry == "lpj":
            rc = lib.pm_gsc_estep_lpj_f64(*head, over.get("logpj", self.logpj.ptr), over.get("ldl", self.logpj.ld), _stream())
        elif self.entry == "blocks":
            rc = lib.pm_gsc_estep_lpj_blocks_f64(*head, over.get("logpj", self.logpj.ptr), over.get("ldl", self.logpj.ld),
                                                 over.get("blocks", self.blocks.ptr), over.get("ldb", self.blocks.ld), _stream())
        else:
            rc = lib.pm_gsc_estep_lists_f64(*head, over.get("nz_idx", self.nz_idx.ptr), over.get("nz_val", self.nz_val.ptr),
                                            over.get("dense_rows", self.dense_rows.ptr),
                                            over.get("dense_count", self.dense_count.ptr), _stream())
        torch.cuda.synchronize()
        return rc

    def inputs_unchanged(self):
        return all(e.unchanged() for e in self.ops.values()) and (self.select or self.cand.unchanged())

    def guards_hold(self):
        return all(e.outside_untouched() for e in self.outs)

    def untouched(self):
        """Nothing was written at all (a refusal, N == 0)."""
        return all(e.unchanged() for e in self.outs) and self.inputs_unchanged()

    def raw(self):
        return self.stats.host().reshape(-1)


def _check_stats(got, start, add, add_abs, rel, widen, H, entry, hot, det, tag, packed=False):
    base = len(add)
    total = start[:base].astype(LD) + add
    scale_of = np.abs(start[:base]).astype(LD) + add_abs
    for sec, sl in R.sections(H, packed).items():
        scale = float(scale_of[sl].max())
        err = float(np.abs(got[sl].astype(LD) - total[sl]).max())
        bound = float(rel) * scale + widen + FLOOR
        _note(entry, ("packed." if packed else "stats.") + sec, hot, det, err, bound)
        assert err <= bound, (tag, sec, err, bound)


def _check_run(run, e, form, hot, tag, thr_p=0.0, mult=None, rows=None, widen=0.0):
    """Everything every E-step call is checked for.  `rows`: the reference row of every datapoint (periodic cases); `mult`:
    how often each reference row occurs."""
    c, det, N = run.c, run.det, run.N
    H = c["H"]
    rows = np.arange(N) if rows is None else rows
    entry = run.entry
    assert run.guards_hold(), (tag, "a guard or padding element of an output was written")
    assert run.inputs_unchanged(), (tag, "an input was written")
    B, rel = _row_bounds(c, e)
    if run.select:
        assert np.array_equal(run.cand.host(), e["cand"][rows]), (tag, "cand")
    assert run.xs.written() and run.xsz.written(), tag
    _close_rows(run.xs.host(), e["xpt_s"][rows], e["xpt_s"].max(axis=1)[rows], rel[rows], entry, "xpt_s", hot, det, tag)
    _close_rows(run.xsz.host(), e["xpt_sz"][rows], e["xsz_abs"].max(axis=1)[rows], rel[rows], entry, "xpt_sz", hot, det, tag)
    got = run.raw()
    base = R.stats_base(H)
    assert not got[base:].any(), (tag, "the scratch tail is not zero again")
    lacc = form in (R.LACC, R.LIST)
    add = R.raw_stats(c, e, lacc, thr_p, mult)
    add_abs = R.raw_stats(c, _abs_of(e), lacc, thr_p, mult)
    zero = np.asarray(add_abs == 0)
    assert np.array_equal(got[:base][zero], run.start[:base][zero]), (tag, "an entry no datapoint contributes to was written",
                                                                      np.nonzero(got[:base][zero] != run.start[:base][zero])[0][:5])
    _check_stats(got, run.start, add, add_abs, float(rel.max()) + N * U, widen, H, entry, hot, det, tag)
    return add, add_abs, rel


def _det_widen(det, run, e, form, thr_p=0.0, mult=None):
    if not det:
        return 0.0
    add_abs = R.raw_stats(run.c, _abs_of(e), form in (R.LACC, R.LIST), thr_p, mult)
    q = _install_quanta(np.abs(run.start[:len(add_abs)]) + add_abs, _addend_max(e), run.N)
    return (run.N + 1) * q / 2


def _check_pack(dev, run, add, add_abs, rel, widen, hot, tag):
    """pm_gsc_pack_stats_f64 on the statistics the run left: equal to the layout's definition applied to those float64 values,
    and within the statistics' bounds of the reference."""
    c, det, H = run.c, run.det, run.c["H"]
    yy = 2.75
    eyy = Emb(np.asarray([yy]), 1, dev)
    out = Emb(np.zeros(2 * H * H + 2 * H + 1), 2 * H * H + 2 * H + 1, dev, fill=False)
    before = run.stats.buf.clone()
    rc = _lib_of(det).pm_gsc_pack_stats_f64(run.stats.ptr, H, eyy.ptr, out.ptr, _stream())
    torch.cuda.synchronize()
    assert rc == PM_OK and out.written() and out.outside_untouched() and eyy.unchanged(), tag
    assert torch.equal(run.stats.buf.view(torch.int64), before.view(torch.int64)), (tag, "pack wrote its input")
    got = out.host()[0]
    raw = run.raw()[:R.stats_base(H)]
    assert np.array_equal(got, R.packed_stats(raw, H, yy)), (tag, "pack is not the documented layout of what it read")
    base = R.stats_base(H)
    total = R.packed_stats(run.start[:base].astype(LD) + add, H, LD(yy))
    total_abs = R.packed_stats(np.abs(run.start[:base]).astype(LD) + add_abs, H, LD(yy))
    _check_stats(got, np.zeros(len(total)), total, total_abs, float(rel.max()) + run.N * U, widen, H, "pack", hot, det, tag, packed=True)


def _check_logpj(run, e, hot, tag, rows=None):
    rows = np.arange(run.N) if rows is None else rows
    B, _ = _row_bounds(run.c, e)
    assert run.logpj.written(), tag
    err = np.abs(run.logpj.host().astype(LD) - e["lp"][rows])
    bound = B[rows]
    i = np.unravel_index(int(np.argmax(err / bound)), err.shape)
    _note(run.entry, "logpj", hot, run.det, err[i], bound[i])
    assert (err <= bound).all(), (tag, "logpj", i, float(err[i]), float(bound[i]))


def _check_blocks(run, e, hot, tag, rows=None):
    """Un-normalised sums of weighted terms: beta B_n relative to the row's largest sum of magnitudes (module docstring)."""
    rows = np.arange(run.N) if rows is None else rows
    c = run.c
    B, _ = _row_bounds(c, e)
    rel = RTOL + LD(c["beta"]) * B.max(axis=1)
    assert run.blocks.written(), tag
    want = e["blocks"][rows]
    _close_rows(run.blocks.host(), want, np.abs(want).max(axis=1), rel[rows], run.entry, "blocks", hot, run.det, tag)


# ----------------------------------------------------------------------------------------------------------- E-step
def _estep_case(dev, name, hot, det, N=None, layouts=("odd",)):
    c, cand, e = _case(name, hot, N)
    p = _assert_cell(det, c, N=N)
    form = p[2]
    for layout in layouts:
        for select in (True, False):
            for sigma0 in (False, True):
                run = Run(dev, det, c, cand, "estep", layout, select, sigma0)
                widen = _det_widen(det, run, e, form)
                tag = (name, hot, det, c["N"], layout, select, sigma0)
                assert run.launch() == PM_OK, tag
                add, add_abs, rel = _check_run(run, e, form, hot, tag, widen=widen)
        _check_pack(dev, run, add, add_abs, rel, widen, hot, tag)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("name", STAT_NAMES)
def test_estep(dev, name, det):
    """Every plain and LACC cell, HOT and COLD: do_select = 1 and 0 (cand handed in, sorted), sigma_sq > 0 (eight table rows,
    the guard pattern behind them) and sigma_sq == 0 (ninth row).  cand by equality, xpt_s / xpt_sz to the row bound, the raw
    statistics by form, the packed ones through pm_gsc_pack_stats_f64.  One case per form also with N = 1 and N = 16, and one in
    all five layouts."""
    for hot in (True, False):
        _estep_case(dev, name, hot, det, layouts=LAYOUTS if name == ALL_LAYOUT_CASE else ("odd",))
        for N in SMALL_N.get(name, ()):
            _estep_case(dev, name, hot, det, N=N)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("name", list(R.EDGE_CASES))
def test_state_trip_edges(dev, name, det):
    """S of 0 (gamma = 1; H' = 1), 1, 15, 16 and 17: the last trip of the state loop empty, full, and one state long (a prefix of
    the full table where no table of that size exists).  state_masks = NULL is legal with S = 0 and PM_EINVAL with S > 0."""
    for hot in (True, False):
        _estep_case(dev, name, hot, det)
    c, cand, e = _case(name, True)
    run = Run(dev, det, c, cand, null_masks=True)
    rc = run.launch()
    if c["S"] == 0:
        assert rc == PM_OK
        _check_run(run, e, _assert_cell(det, c)[2], True, (name, "NULL masks"), widen=_det_widen(det, run, e, R.LACC))
    else:
        assert rc == PM_EINVAL and run.untouched(), (name, rc)


# ------------------------------------------------------------------------------------------------------- log-joints
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("name", LPJ_NAMES)
def test_estep_lpj(dev, name, det):
    """Every LPJ cell: logpj covers the null state, the singletons and the multi-cause states in table order, on a padded
    ldl; xpt_s, xpt_sz and the statistics are those of the statistics form of the same operands (checked against the same
    reference to the same bound, from both entry points)."""
    for hot in (True, False):
        for N in (None,) + SMALL_N.get(name, ()):
            c, cand, e = _case(name, hot, N)
            p = _assert_cell(det, c, N=N)
            for select, sigma0 in ((True, False), (False, True)):
                run = Run(dev, det, c, cand, "lpj", "odd", select, sigma0)
                widen = _det_widen(det, run, e, R.LPJ)
                tag = (name, hot, det, c["N"], select, sigma0)
                assert run.launch() == PM_OK, tag
                add, add_abs, rel = _check_run(run, e, R.LPJ, hot, tag, widen=widen)
                _check_logpj(run, e, hot, tag)
            _check_pack(dev, run, add, add_abs, rel, widen, hot, tag)
            ps = _assert_cell(det, c, flags=0, N=N)
            run = Run(dev, det, c, cand, "estep", "even", True, False)
            widen = _det_widen(det, run, e, ps[2])
            assert run.launch() == PM_OK, tag
            _check_run(run, e, ps[2], hot, tag + ("statistics form",), widen=widen)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("name", LPJ_NAMES[::3] + ["l_v1_g2p"])
def test_estep_lpj_blocks(dev, name, det):
    """pm_gsc_estep_lpj_blocks_f64 on padded ldl and ldb: the blocks are the un-normalised sums over the multi-cause states in
    `cand` order; everything else as the LPJ form leaves it."""
    for hot in (True, False):
        c, cand, e = _case(name, hot)
        _assert_cell(det, c, flags=R.F_LPJ | R.F_BLOCKS)
        for layout, select in (("odd", True), ("mix_a", False)):
            run = Run(dev, det, c, cand, "blocks", layout, select, False)
            widen = _det_widen(det, run, e, R.LPJ)
            tag = (name, hot, det, layout, select)
            assert run.launch() == PM_OK, tag
            _check_run(run, e, R.LPJ, hot, tag, widen=widen)
            _check_logpj(run, e, hot, tag)
            _check_blocks(run, e, hot, tag)


# ------------------------------------------------------------------------------------------------------ second trip
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("name,entry", [("p_v1_g2", "estep"), ("a_v1_g3", "estep"), ("l_v1_g3", "lpj"), ("t_v8_g2", "lists")])
def test_second_trip(dev, name, entry, det):
    """N = 16 (grid cap + 3) + 5 datapoints: every workgroup walks a second group of sixteen (three of them a third, and the
    last group is ragged), so a datapoint's pair blocks are sent at the top of its row's NEXT datapoint with the normaliser kept
    from before, and the last one's after the loop.  Rows beyond the first 64 are copies of the first 64 (shifted by five per
    trip, so that a workgroup's second trip holds other rows than its first); the reference is computed on the distinct rows
    and the statistics count each with its multiplicity."""
    for hot in (True, False):
        c, cand, e = _case(name, hot, 64)
        cap = 3 * _cus()
        N = 16 * (cap + 3) + 5
        # (16 cap may be a multiple of 64 -- it is at 256 CUs: without the shift a workgroup would meet the SAME rows on its
        # second trip, and a normaliser or candidate set kept from the wrong trip would go unseen)
        rows = (np.arange(N) + 5 * (np.arange(N) // (16 * cap))) % 64
        mult = np.bincount(rows, minlength=64)
        p = _assert_cell(det, c, N=N)
        assert p[4] == cap and p[5] >= 2, p
        tables = c["tables"]
        if entry == "lists":
            row, thr = R.thr_for_count(e["xpt_s"], e["xpt_sz"], 16)
            tables = R.with_thresholds(c["tables"], thr=thr)
        run = Run(dev, det, c, cand[rows], entry, "odd", True, False, tables=tables, scores=c["scores"][rows],
                  ynorm2=c["ynorm2"][rows])
        widen = _det_widen(det, run, e, p[2], mult=mult)
        tag = (name, hot, det, N)
        assert run.launch() == PM_OK, tag
        _check_run(run, e, p[2], hot, tag, mult=mult, rows=rows, widen=widen)
        if entry == "lpj":
            _check_logpj(run, e, hot, tag, rows=rows)
        if entry == "lists":
            _check_lists(run, e, thr, hot, tag, rows=rows)


# ---------------------------------------------------------------------------------------------------------- selection
SELECTION_SHAPES = [(1, 1), (16, 3), (17, 10), (32, 5), (33, 2), (64, 9), (65, 10), (128, 7), (129, 3), (256, 9), (257, 4),
                    (512, 6)]


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("H,Hp", SELECTION_SHAPES)
def test_selection(dev, H, Hp, det):
    """Exact scores (tests/test_gsc_kernels_cpu.py::test_selection_scores_are_exact) at both ends of every VPL bucket: ties at the
    cut and inside the selected set resolve towards the larger index; rows of all +0.0 and all -0.0 (keys that are subnormals
    differing in the index bits alone); rows whose clamps give 0 (from +inf) and -DBL_MAX (from NaN and from -inf).  Every
    selected row is strictly increasing and within [0, H).  (The statistics of the NaN rows are NaN: only `cand` is compared.)"""
    for c in (R.make_selection_case(H, Hp), R.make_zero_case(H, Hp, False), R.make_zero_case(H, Hp, True)):
        want = R.select(c)
        run = Run(dev, det, c, np.zeros_like(want), "estep", "odd", True, False)
        assert run.launch() == PM_OK, c["name"]
        got = run.cand.host()
        assert (np.diff(got, axis=1) > 0).all() and got.min() >= 0 and got.max() < H, (c["name"], got)
        assert np.array_equal(got, want), (c["name"], np.nonzero((got != want).any(axis=1))[0])
        assert run.guards_hold() and run.inputs_unchanged(), c["name"]


@pytest.mark.parametrize("det", [False, True])
def test_component_scores(dev, det):
    """pm_gsc_component_scores_f64 on a padded ldo: equal to the reference on the exact inputs of the selection cases, clamp rows
    included (their ranking values are what test_selection's candidates were chosen on); to the log-joint bound on real-valued
    cases."""
    lib = _lib_of(det)
    for k, (H, Hp) in enumerate(SELECTION_SHAPES):
        for c in (R.make_selection_case(H, Hp), R.make_zero_case(H, Hp, True)):
            N = c["N"]
            layout = LAYOUTS[k % len(LAYOUTS)]
            es, ey, et = Emb(c["scores"], _ld(H, layout, 0), dev), Emb(c["ynorm2"], N, dev), Emb(c["tables"][:4].reshape(-1), 4 * H, dev)
            eo = Emb(np.zeros((N, H)), _ld(H, layout, 1) + 2, dev, fill=False)
            rc = lib.pm_gsc_component_scores_f64(es.ptr, es.ld, ey.ptr, et.ptr, ctypes.c_double(c["sigma_sq"]), N, H, eo.ptr, eo.ld,
                                                 _stream())
            torch.cuda.synchronize()
            want = R.component_scores(c)
            got = eo.host()
            assert rc == PM_OK and np.array_equal(got.view(np.int64), want.view(np.int64)), (c["name"], layout)
            assert eo.outside_untouched() and es.unchanged() and ey.unchanged() and et.unchanged(), c["name"]
    for name in ("a_v4_g3", "p_v32_g3"):
        for hot in (True, False):
            c, cand, e = _case(name, hot)
            N, H = c["N"], c["H"]
            es, ey, et = Emb(c["scores"], H + 3, dev), Emb(c["ynorm2"], N, dev), Emb(c["tables"][:4].reshape(-1), 4 * H, dev)
            eo = Emb(np.zeros((N, H)), H + 1, dev, fill=False)
            rc = lib.pm_gsc_component_scores_f64(es.ptr, es.ld, ey.ptr, et.ptr, ctypes.c_double(c["sigma_sq"]), N, H, eo.ptr, eo.ld,
                                                 _stream())
            torch.cuda.synchronize()
            assert rc == PM_OK and eo.written() and eo.outside_untouched() and es.unchanged(), name
            want = R.component_scores(c).astype(LD)
            B, _ = _row_bounds(c, e)
            err = np.abs(eo.host().astype(LD) - want)
            assert (err <= B[:, 1:1 + H]).all(), (name, hot, float((err / B[:, 1:1 + H]).max()))
            _note("component_scores", "scores", hot, det, float(err.max()), float(B[:, 1:1 + H].max()))


# ---------------------------------------------------------------------------------------------------------- thresholds
@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("name", R.THRESHOLD_CASES + (R.H2_CASE,))
def test_pair_threshold(dev, name, det):
    """tables[8 H + 2] = thr_p three ways: 0; set between two reference values (tests/test_gsc_kernels_cpu.py: none within
    1 +- 2^-20 of it) with sigma_sq == 0, where an entry of a datapoint's blocks is sent when vss > thr_p resp. |vzz| > thr_p and
    the LACC form always keeps the diagonal; set but sigma_sq != 0, where nothing is dropped (and the ninth row is not even
    handed in).  At H = 2 thr_p is ignored (the table has no such entry: the guard pattern follows)."""
    for hot in (True, False):
        c, cand, e = _case(name, hot)
        entry = "lpj" if c["flags"] & R.F_LPJ else "estep"
        form = _assert_cell(det, c)[2]
        thr_p = R.pick_thr_p(e) if c["H"] > 2 else 0.0
        ways = [(0.0, True, 0.0), (thr_p, True, thr_p), (thr_p, False, 0.0)] if c["H"] > 2 else [(0.0, True, 0.0), (0.0, False, 0.0)]
        for given, sigma0, effective in ways:
            tables = R.with_thresholds(c["tables"], thr_p=given) if c["H"] > 2 else c["tables"]
            run = Run(dev, det, c, cand, entry, "odd", True, sigma0, tables=tables)
            widen = _det_widen(det, run, e, form, thr_p=effective)
            tag = (name, hot, det, given, sigma0)
            assert run.launch() == PM_OK, tag
            _check_run(run, e, form, hot, tag, thr_p=effective, widen=widen)
            if effective:
                dropped = R.raw_stats(c, _abs_of(e), form == R.LACC, 0.0) != R.raw_stats(c, _abs_of(e), form == R.LACC, effective)
                assert dropped.any(), (tag, "the threshold drops nothing")


# --------------------------------------------------------------------------------------------------------------- lists
def _check_lists(run, e, thr, hot, tag, rows=None):
    N = run.N
    rows = np.arange(N) if rows is None else rows
    idx, vz, vs, written, dense, nsig = R.list_split(e["xpt_s"], e["xpt_sz"], thr)
    _, rel = _row_bounds(run.c, e)
    got_idx = run.nz_idx.host().view(np.uint16)
    assert np.array_equal(got_idx, idx[rows]), (tag, "nz_idx", np.nonzero((got_idx != idx[rows]).any(axis=1))[0][:5])
    val = run.nz_val.host()
    raw = run.nz_val.block().cpu().numpy().view(np.int64)
    w = np.concatenate([written[rows], written[rows]])
    assert (raw[~w] == run.nz_val.sent).all(), (tag, "a value slot behind a terminator was written")
    assert (raw[w] != run.nz_val.sent).all(), (tag, "a listed value was not written")
    for plane, want, scale, what in ((val[:N], vz[rows], e["xsz_abs"].max(axis=1)[rows], "nz_val.sz"),
                                      (val[N:], vs[rows], e["xpt_s"].max(axis=1)[rows], "nz_val.s")):
        _close_rows(np.where(written[rows], plane, 0.0), want, scale, rel[rows], run.entry, what, hot, run.det, tag)
    want_dense = np.nonzero(np.isin(rows, dense))[0]
    count = int(run.dense_count.host()[0, 0])
    assert count == len(want_dense), (tag, "dense_count", count, len(want_dense))
    dr = run.dense_rows.block().cpu().numpy().reshape(-1)
    assert sorted(dr[:count].tolist()) == want_dense.tolist(), (tag, "dense_rows")
    assert (dr[count:] == run.dense_rows.sent).all(), (tag, "dense_rows behind the count")
    return nsig


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("name", LIST_NAMES)
def test_lists(dev, name, det):
    """All four LIST cells, with thr = 0 (every row dense, *dense_count == N, 0xFFFF in all sixteen slots) and thr set so that
    some row has exactly 0, 1, 16 and 17 significant entries (16: the longest list; 17: the shortest dense row): indices in
    latent order with 0xFFFF behind the last, both planes of nz_val, value slots behind the terminator untouched, dense rows as
    a set; xpt_s, xpt_sz and stats are those of the non-LIST run of the same operands (same reference, same bound)."""
    for hot in (True, False):
        for N in (None,) + SMALL_N.get(name, ()):
            c, cand, e = _case(name, hot, N)
            p = _assert_cell(det, c, N=N)
            todo = [(None, 0.0)] + ([(k, None) for k in (0, 1, 16, 17)] if N is None else [(1, None)])
            for k, thr in todo:
                row = None
                if thr is None:
                    row, thr = R.thr_for_count(e["xpt_s"], e["xpt_sz"], k)
                run = Run(dev, det, c, cand, "lists", "odd", k != 16, k == 17, tables=R.with_thresholds(c["tables"], thr=thr))
                widen = _det_widen(det, run, e, R.LIST)
                tag = (name, hot, det, c["N"], k)
                assert run.launch() == PM_OK, tag
                _check_run(run, e, R.LIST, hot, tag, widen=widen)
                nsig = _check_lists(run, e, thr, hot, tag)
                if k is None:
                    assert int(run.dense_count.host()[0, 0]) == c["N"], tag
                    assert (run.nz_idx.host().view(np.uint16) == 0xFFFF).all(), tag
                else:
                    assert nsig[row] == k, tag
            ps = _assert_cell(det, c, flags=0, N=N)
            run = Run(dev, det, c, cand, "estep", "even", True, False)
            widen = _det_widen(det, run, e, ps[2])
            assert run.launch() == PM_OK, name
            _check_run(run, e, ps[2], hot, (name, hot, det, "statistics form"), widen=widen)


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("H", sorted(R.LIST_PAIRS_CELLS))
def test_list_pairs(dev, H, det):
    """H of 64, 128, 192 (three chunks of 64 rows) and 256: lists of every length 0 .. 16 (the magic division p / cnt for every
    cnt), NaN in every value slot behind a terminator, N = 45 < 64 (one ragged group), `out` starting from multiples of 1/8:
    with integer values every sum is exact in any order -- equality."""
    N = 45
    rc, p = _plan(det, R.LIST_PAIRS, H, 0, 0, 0, 0, 0, N)
    assert rc == PM_OK and p[7:11] == R.LIST_PAIRS_CELLS[H], p
    rng = np.random.RandomState(H)
    idx = np.full((N, R.NZ_MAX), 0xFFFF, dtype=np.uint16)
    vs = np.full((N, R.NZ_MAX), np.nan)
    vz = np.full((N, R.NZ_MAX), np.nan)
    for r in range(N):
        k = r % 17
        idx[r, :k] = np.sort(rng.permutation(H)[:k])
        vs[r, :k] = rng.randint(0, 5, size=k)
        vz[r, :k] = rng.randint(-4, 5, size=k)
    idx[3, :3] = [0, 31, H - 1]
    start = (1 + (np.arange(2 * H * H) * 3) % 8) / 8.0
    want = (start.astype(LD) + R.list_pairs(idx, vs, vz, H)).astype(np.float64)
    ei, es, ez = Emb(idx.view(np.int16), R.NZ_MAX, dev), Emb(vs, R.NZ_MAX, dev), Emb(vz, R.NZ_MAX, dev)
    eo = Emb(start.reshape(2 * H, H), H, dev)
    rc = _lib_of(det).pm_gsc_list_pairs_f64(ei.ptr, es.ptr, ez.ptr, N, H, eo.ptr, _stream())
    torch.cuda.synchronize()
    got = eo.host().reshape(-1)
    assert rc == PM_OK and np.array_equal(got, want), (H, det, np.nonzero(got != want)[0][:8])
    assert eo.outside_untouched() and ei.unchanged() and es.unchanged() and ez.unchanged()


# --------------------------------------------------------------------------------------------------- row permutation
@pytest.mark.parametrize("name", ["l_v1_g3", "l_v8_g6"])
def test_row_permutation(dev, name):
    """A datapoint's cand, xpt_s, xpt_sz, logpj and blocks depend on its own row and the parameters only: permuting the
    datapoints permutes them bit for bit."""
    for hot in (True, False):
        c, cand, e = _case(name, hot)
        perm = np.random.RandomState(5).permutation(c["N"])
        a = Run(dev, False, c, cand, "blocks", "odd", True, False)
        b = Run(dev, False, c, cand[perm], "blocks", "odd", True, False, scores=c["scores"][perm], ynorm2=c["ynorm2"][perm])
        assert a.launch() == PM_OK and b.launch() == PM_OK
        for x, y in ((a.cand, b.cand), (a.xs, b.xs), (a.xsz, b.xsz), (a.logpj, b.logpj), (a.blocks, b.blocks)):
            hx, hy = x.host(), y.host()
            v = np.int32 if hx.dtype == np.int32 else np.int64
            assert np.array_equal(hx[perm].view(v), hy.view(v)), (name, hot)


# --------------------------------------------------------------------------------------------------- return codes
@pytest.mark.parametrize("det", [False, True])
def test_return_codes(dev, det):
    """Every PM_EINVAL / PM_ERANGE condition of the launchers, with every output still holding its start pattern, and N == 0:
    PM_OK, nothing touched."""
    c, cand, e = _case("a_v8_g3", True)
    H, Hp, S, N = c["H"], c["Hp"], c["S"], c["N"]
    K, B = 1 + H + S, 2 * Hp * Hp + 2 * Hp + 1
    big = dict(lds=1 << 20, ldx=1 << 20, ldl=1 << 20, ldb=1 << 20)      # (so that the leading-dimension checks pass first)
    common = [(dict(scores=None), PM_EINVAL), (dict(gram=None), PM_EINVAL), (dict(psi=None), PM_EINVAL), (dict(yn=None), PM_EINVAL),
              (dict(tables=None), PM_EINVAL), (dict(cand=None), PM_EINVAL), (dict(xs=None), PM_EINVAL), (dict(xsz=None), PM_EINVAL),
              (dict(stats=None), PM_EINVAL), (dict(N=-1), PM_EINVAL), (dict(H=0), PM_EINVAL), (dict(Hp=0), PM_EINVAL),
              (dict(S=-1), PM_EINVAL), (dict(lds=H - 1), PM_EINVAL), (dict(ldx=H - 1), PM_EINVAL), (dict(masks=None), PM_EINVAL),
              (dict(sigma_sq=-1.0), PM_EINVAL), (dict(sigma_sq=float("nan")), PM_EINVAL),
              (dict(gamma=9), PM_ERANGE), (dict(gamma=0), PM_ERANGE), (dict(Hp=17, **big), PM_ERANGE),
              (dict(H=513, **big), PM_ERANGE), (dict(Hp=9, H=8, **big), PM_ERANGE), (dict(S=40000, **big), PM_ERANGE),
              (dict(N=0), PM_OK)]
    extra = {"estep": [],
             "lpj": [(dict(logpj=None), PM_EINVAL), (dict(ldl=K - 1), PM_EINVAL)],
             "blocks": [(dict(logpj=None), PM_EINVAL), (dict(blocks=None), PM_EINVAL), (dict(ldb=B - 1), PM_EINVAL),
                        (dict(ldl=K - 1), PM_EINVAL)],
             "lists": [(dict(nz_idx=None), PM_EINVAL), (dict(nz_val=None), PM_EINVAL), (dict(dense_rows=None), PM_EINVAL),
                       (dict(dense_count=None), PM_EINVAL), (dict(gamma=4), PM_ERANGE), (dict(H=64), PM_ERANGE),
                       (dict(H=257, **big), PM_ERANGE), (dict(Hp=9, S=36, gamma=2), PM_ERANGE)]}
    for entry in ("estep", "lpj", "blocks", "lists"):
        run = Run(dev, det, c, cand, entry, "odd", True, entry == "lists")
        for over, want in common + extra[entry]:
            rc = run.launch(**over)
            assert rc == want and run.untouched(), (entry, over, rc)
    lib = _lib_of(det)
    # pm_gsc_list_pairs_f64
    idx = Emb(np.full((4, R.NZ_MAX), -1, dtype=np.int16), R.NZ_MAX, dev)
    v = Emb(np.zeros((4, R.NZ_MAX)), R.NZ_MAX, dev)
    o = Emb(np.ones((2 * 64, 64)), 64, dev)
    for a, want in (((None, v.ptr, v.ptr, 4, 64, o.ptr), PM_EINVAL), ((idx.ptr, None, v.ptr, 4, 64, o.ptr), PM_EINVAL),
                    ((idx.ptr, v.ptr, None, 4, 64, o.ptr), PM_EINVAL), ((idx.ptr, v.ptr, v.ptr, 4, 64, None), PM_EINVAL),
                    ((idx.ptr, v.ptr, v.ptr, -1, 64, o.ptr), PM_EINVAL), ((idx.ptr, v.ptr, v.ptr, 4, 0, o.ptr), PM_EINVAL),
                    ((idx.ptr, v.ptr, v.ptr, 4, 320, o.ptr), PM_ERANGE), ((idx.ptr, v.ptr, v.ptr, 4, 100, o.ptr), PM_ERANGE),
                    ((idx.ptr, v.ptr, v.ptr, 0, 64, o.ptr), PM_OK), ((idx.ptr, v.ptr, v.ptr, 0, 100, o.ptr), PM_ERANGE)):
        rc = lib.pm_gsc_list_pairs_f64(*a, _stream())
        torch.cuda.synchronize()
        assert rc == want and o.unchanged() and idx.unchanged(), ("list_pairs", a[3:5], rc)
    # pm_gsc_pack_stats_f64
    st, yy, out = Emb(np.ones(R.stats_base(4)), R.stats_base(4), dev), Emb(np.ones(1), 1, dev), Emb(np.zeros(41), 41, dev, fill=False)
    for a, want in (((None, 4, yy.ptr, out.ptr), PM_EINVAL), ((st.ptr, 4, None, out.ptr), PM_EINVAL), ((st.ptr, 4, yy.ptr, None), PM_EINVAL),
                    ((st.ptr, 0, yy.ptr, out.ptr), PM_EINVAL), ((st.ptr, 513, yy.ptr, out.ptr), PM_ERANGE)):
        rc = lib.pm_gsc_pack_stats_f64(*a, _stream())
        torch.cuda.synchronize()
        assert rc == want and out.unchanged() and st.unchanged(), ("pack", rc)
    # pm_gsc_component_scores_f64
    sc, yn, tb = Emb(np.ones((3, 5)), 6, dev), Emb(np.ones(3), 3, dev), Emb(np.ones(20), 20, dev)
    out = Emb(np.zeros((3, 5)), 7, dev, fill=False)
    ok = dict(scores=sc.ptr, lds=6, yn=yn.ptr, tables=tb.ptr, s2=1.0, N=3, H=5, out=out.ptr, ldo=7)
    for over, want in ((dict(scores=None), PM_EINVAL), (dict(yn=None), PM_EINVAL), (dict(tables=None), PM_EINVAL),
                       (dict(out=None), PM_EINVAL), (dict(N=-1), PM_EINVAL), (dict(H=0), PM_EINVAL), (dict(lds=4), PM_EINVAL),
                       (dict(ldo=4), PM_EINVAL), (dict(s2=0.0), PM_EINVAL), (dict(s2=float("nan")), PM_EINVAL), (dict(N=0), PM_OK),
                       (dict(N=1 << 41, H=512, lds=512, ldo=512), PM_ERANGE)):
        a = dict(ok, **over)
        rc = lib.pm_gsc_component_scores_f64(a["scores"], a["lds"], a["yn"], a["tables"], ctypes.c_double(a["s2"]), a["N"], a["H"],
                                             a["out"], a["ldo"], _stream())
        torch.cuda.synchronize()
        assert rc == want and out.unchanged(), ("component_scores", over, rc)


@pytest.fixture(scope="module", autouse=True)
def _report_worst_errors():
    """After the module's tests: the largest error of every bounded comparison that ran, per entry, quantity, HOT / COLD and
    library (-s shows it).  Not a check of its own: each comparison asserted its bound where it was made."""
    yield
    for key in sorted(WORST):
        ratio, err, bound = WORST[key]
        print("worst %-16s %-14s %-4s %-7s err %.3e  bound %.3e  ratio %.2e" % (key + (err, bound, ratio)))
