"""The kernels that run between the E-step and the M-step, through the C ABI, on padded, pattern-guarded operands, from both
libraries, against the plain reference tests/select_kernels_reference.py (pinned on the CPU by tests/test_select_kernels_cpu.py):
  infer_kernels.hip   pm_infer_topk_f64, pm_infer_topk_cols_f64, pm_infer_topk_signed_f64
  kth_select.hip      pm_kth_hist_f64, pm_kth_scan, pm_kth_value_f64, pm_kth_round_f64, pm_kth_round_k_f64, pm_kth_final_f64,
                      pm_kth_final_z_f64
  spd_inverse.hip     pm_spd_inverse_f64, pm_spd_inverse_batch_f64, pm_spd_inverse_warm_f64, pm_spd_inverse_warm_long_f64,
                      pm_spd_inverse_warm_batch_f64, pm_inverse_warm_batch_f64 (with pm_spd_inverse_warm_work_len)

Harness: ``Emb`` of tests/test_eval_kernels_gpu.py, with int8 (0x5A), uint16 (0xA5A5) and int64 / uint64 (0x5EADBEEF5EADBEEF)
added in the subclass ``EmbX``.  Every operand sits in a buffer with 16 guard rows before and after and a padded leading
dimension wherever the ABI has one (ldl, ldm; ldu, ldo and the batch strides, whose gaps hold the pattern too).  top_idx,
top_lpc, top_rel, top_post, tie, s_out, m_out, am_out, states, hists, out, work, pivots and accepted have no leading dimension:
they are exactly as long as the header says, guards around them.  After every call: guards and padding of every output still
hold the pattern, every input is bit-unchanged, the result block is written where the contract says it is and still holds the
pattern where the contract leaves it.  Every entry is called twice from each library; the four results must be bit-equal (the
only atomics are integer ones).  The only invalid arguments passed are those the launchers reject before launching.
No case is excluded from any comparison.

Equality (value for value; non-finite values by kind): top_idx, tie, s_out, top_rel (v - max is one correctly rounded
operation) of every row; top_lpc, the non-candidate marginals and the candidate marginals with a single non-negligible term of
the exact-class rows (one dominant entry, everything else -inf or >= 64 below: K exp(-64) < 2^-54, so the log-sum-exp IS the
maximum whatever the order of summation -- asserted on the CPU); the signed / absolute marginal at the positions where the
dominant state of such a row is non-zero (+-1 / 1); every state, histogram and value of the radix select; `full`, and on the
exact SPD case (A = L D L^T, dyadic: every intermediate of the sweep is a float64 in any evaluation order, asserted on the CPU
in Fractions) `inv` and the pivots.

Bounded, against the longdouble reference (RTOL = 1e-11 of tests/test_eval_kernels_gpu.py, the project's bound for everything
that goes through libm's exp and log; not fitted):
  top_lpc, top_post, marg   |err| <= RTOL (1 + |lse| + |value|): lse = max + log(sum exp) rounds a handful of times on a sum in
             [1, K], v - lse once more; exp of it has that error relatively (|.| <= 1).  A wrong column or a dropped term is
             orders of magnitude above it at the +-20 spread of the generic rows.
  m, am      RTOL sum_s p_s |v_sj| + 1e-290: every term has relative error <= RTOL's share, the sum of S terms adds S u.
  inverses   as tests/test_bsc_gpu.py: atol = 1e-14 cond max|ref| for the sweep and an accepted refinement, 1e-13 for the long
             entry, pivots rtol 1e-9 (sweep) / 1e-7 (refinement), the accept / reject logic of test_spd_inverse_warm.

Worst observed error as a fraction of its bound (MI355X; 52 tests pass on the unchanged kernels in 9.2 s, the slowest --
test_infer_topk_signed[s3big], 16389 rows -- in 1.1 s, then test_spd_inverse_warm_layouts[255] 1.0 s and
test_infer_topk_cols[k3big] 1.0 s; the module's autouse fixture prints the table with -s).  Both libraries give the same bits in
every call, so the two columns are equal:
                                         default    deterministic
  topk       top_lpc                     1.6e-5     1.6e-5
  topk       marg                        1.6e-5     1.6e-5
  signed     top_lpc                     1.6e-5     1.6e-5
  signed     top_post                    5.9e-6     5.9e-6
  signed     m                           3.4e-4     3.4e-4
  signed     am                          3.5e-4     3.5e-4
  sweep      inv                         0.022      0.022
  sweep      pivots                      1.1e-6     1.1e-6
  warm       inv                         0.012      0.012
  warm       pivots                      7.1e-9     7.1e-9
  warm       pivots[0], exact case       0          0
  warm_long  inv                         0.0013     0.0013
Nothing exceeds its bound and no test of this module fails on the unchanged source: no kernel bug was found.  The RTOL-based
bounds (libm) are four to five orders of magnitude wide, as in the other kernel-test modules; everything that decides an index, a
flag, a state or a digit is compared with equality.

Mutants, one line each, values and predicates only (a leading dimension or stride replaced by the width still reads and writes
inside the same padded buffer; none changes a launch shape), each built into a library of its own outside the tree and run once
against this module on the MI355X, its entries of the mutated file in place of both libraries':
 infer_kernels.hip
   1  `k > bi` -> `k < bi` (first kernel)                    8 fail: test_infer_topk_cols, every case but k2
   2  `oi > idx` -> `oi < idx` in pm_wave_argmax             13: test_infer_topk_cols but k2; test_infer_topk_signed[s64, s65, s130, s130d, s3big]
   3  `n * ldl` -> `n * K` (first kernel)                    8: test_infer_topk_cols, every case with N > 1
   4  `n * ldm` -> `n * H`                                   8: the same
   5a `n += nwaves` -> leaves the loop (first kernel)        1: test_infer_topk_cols[k3big]
   5b the same in the signed kernel                          1: test_infer_topk_signed[s3big]
   6  `r <= topK` -> `r < topK`                              2: test_infer_topk_signed[s130, s130d] (the rows tied across the cut)
   7  the `(bv - lse) == (pv - lse)` clause dropped          7: test_infer_topk_signed, every case (the normalised-only tie)
   8  `moff = 1 + single_cols` -> `1 + H`                    4: test_infer_topk_cols[k63, k129, k200, k200b] (single_cols = 2 H, 3 H)
   9  `>> j` -> `>> (j & 7)`                                 3: test_infer_topk_cols[k65, k200, k200b] (H' = 16)
  10  the position loop of s_out reversed                    6: test_infer_topk_signed[s64, s65eq, s130, s130d], ..._given_indices (both)
 kth_select.hip
   1a the grid-stride increment of kth_hist_kernel -> leaves the loop     1: test_kth_select[big]
   1b the same in kth_round_kernel                           1: test_kth_select[big]
   2a `>= k` -> `> k` in the chunk pick of kth_scan_block    7: test_kth_select (all six), test_kth_rezero_and_second_select
   2b `>= k` -> `> k` in its in-chunk pick                   7: the same
   3  `above - c0` -> `above`                                2: test_kth_select[digits0, specials] -- the rank past the end (k = n + 3) with keys in
                                                             chunk 0; it SURVIVED every k in 1 .. n (some chunk always qualifies): that case was added
   4  rezero bound `rounds * BINS` -> `BINS`                 1: test_kth_rezero_and_second_select
   5  `~b` -> `b ^ (1ull << 63)` in key_of                   3: test_kth_select[digits0, specials, big] (the sets with negative values)
 spd_inverse.hip
   1  `ldu` -> `n` in the sweep's load                       11: test_spd_inverse_layouts (n > 1), test_spd_inverse_exact_case, ..._warm_nan_start
   2  `ldo` -> `n` in its store                              9: test_spd_inverse_layouts (n > 1), test_spd_inverse_exact_case
   3  `stride_prev` -> `n * n` in launch_warm                15: test_spd_inverse_warm_layouts, test_inverse_warm_general_masks, ..._exact_case, ..._nan_start
   4  `gen` forced to false in ns_finish_kernel              2: test_inverse_warm_general_masks (both)
   5  `(r2 < guard_tol2)` -> `!(r2 >= guard_tol2)`           2: test_spd_inverse_warm_nan_start (both)
All 23 fail; none survives.
"""
import numpy as np
import pytest

import select_kernels_reference as R
from test_eval_kernels_gpu import GUARD_ROWS, LAYOUTS, RTOL, SENT_F64, Emb, _ld, _stream, dev  # noqa: F401
from test_mixture_kernels_gpu import _all_equal, _bits, _f, _lib_of, _pattern_equal, _same_bits

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PM_OK, PM_EINVAL, PM_ERANGE = 0, -1, -2
LD = np.longdouble
FLOOR = 1e-290
LIBS = (False, True)
WORST = {}
PATTERN = np.array([SENT_F64], dtype=np.uint64).view(np.float64)[0]
SENT_I8, SENT_U16, SENT_I64 = 0x5A, 0xA5A5, 0x5EADBEEF5EADBEEF
GAP = R.GAP


class EmbX(Emb):
    """Emb with the element types these kernels add: int8, uint16 (kept as int16 bits) and int64 / uint64 (kept as int64 bits)."""
    _TYPES = dict(Emb._TYPES)
    _TYPES.update({np.dtype(np.int8): (torch.int8, SENT_I8), np.dtype(np.int16): (torch.int16, SENT_U16 - 0x10000),
                   np.dtype(np.int64): (torch.int64, SENT_I64)})
    _AS = {np.dtype(np.uint16): np.int16, np.dtype(np.uint64): np.int64}

    def __init__(self, array, ld, dev, off=0, fill=True):
        a = np.asarray(array)
        self.np_dtype = a.dtype
        if a.dtype in self._AS:
            a = np.ascontiguousarray(a).view(self._AS[a.dtype])
        super().__init__(a, ld, dev, off=off, fill=fill)

    def host(self):
        return np.ascontiguousarray(super().host()).view(self.np_dtype)


def _note(entry, what, det, err, bound):
    key = (entry, what, "det" if det else "default")
    ratio = float(err) / float(bound) if bound > 0 else 0.0
    if ratio > WORST.get(key, (-1.0, 0.0, 0.0))[0]:
        WORST[key] = (ratio, float(err), float(bound))


def _exact(got, want, tag, where=None):
    """Equality with the reference where it is finite (and `where` holds); the same kind of non-finite value elsewhere."""
    fin = _pattern_equal(got, want, tag)
    w = _f(want)
    sel = fin if where is None else fin & where
    assert np.array_equal(np.asarray(got)[sel], w[sel]), (tag, "not equal to the reference at", np.argwhere(sel & (np.asarray(got) != w))[:8])


def _bounded(got, want, bound, entry, what, det, tag):
    fin = _pattern_equal(got, want, tag)
    if not fin.any():
        return
    g, w = np.asarray(got).astype(LD)[fin], np.asarray(want, dtype=LD)[fin]
    b = np.broadcast_to(np.asarray(bound, dtype=LD), np.shape(got))[fin]
    assert np.isfinite(_f(b)).all() and (b > 0).all(), (tag, what, "a bound is not a positive finite number")
    err = np.abs(g - w)
    i = int(np.argmax(err / b))
    _note(entry, what, det, err[i], b[i])
    assert (err <= b).all(), (tag, what, "error", float(err[i]), "bound", float(b[i]), "at", np.argwhere(fin)[i])


def _vec(x, dev, fill=True):
    return EmbX(np.asarray(x), max(len(x), 1), dev, fill=fill)


def _mat(x, dev, fill=True):
    """A dense matrix without a leading dimension of its own in the ABI: guards before and after only."""
    x = np.asarray(x)
    return EmbX(x.reshape(x.shape[0], -1), int(np.prod(x.shape[1:])), dev, fill=fill)


def _finish(rc, tag, outs, ins, unwritten=()):
    torch.cuda.synchronize()
    assert rc == PM_OK, (tag, rc)
    for k, e in outs.items():
        assert e.outside_untouched(), (tag, k, "a guard or padding element was written")
        assert k in unwritten or e.written(), (tag, k, "an element of the result was not written")
    for k, e in ins.items():
        assert e.unchanged(), (tag, k, "an input was written")


def _rejected(rc, want, tag, outs, ins):
    """A launcher's refusal: the code, and not a bit of any operand changed."""
    torch.cuda.synchronize()
    assert rc == want, (tag, rc, want)
    assert all(e.unchanged() for e in list(outs.values()) + list(ins.values())), (tag, "a rejected call wrote something")


def _two_layouts(all_layouts):
    return LAYOUTS if all_layouts else ("tight", "odd")


# =========================================================================== pm_infer_topk_cols_f64 / pm_infer_topk_f64
# name: (H, Hp, S, single_cols / H, N, topKs, every layout, first row kind)
TOPK_CASES = {
    "k2":    (1, 1, 0, 1, 3, (1, 2), False, 0),
    "k63":   (10, 4, 42, 2, 4, (1, 5, 63), False, 2),
    "k64":   (12, 1, 51, 1, 5, (1, 5, 64), False, 5),
    "k65":   (16, 16, 48, 1, 9, (1, 5, 65), True, 0),
    "k129":  (20, 4, 68, 3, 9, (1, 5, 70, 129), False, 1),
    "k200":  (30, 16, 139, 2, 5, (5, 200), False, 4),
    "k200b": (30, 16, 139, 2, 5, (1, 5), False, 9),
    "k129n1": (20, 4, 68, 3, 1, (5,), False, 3),
    "k3big": (1, 1, 1, 1, 16384 + 5, (1, 3), False, 0),
}
ROW_KINDS = ("exact", "tie64", "tieadj", "alleq", "tiecut", "ninf", "generic", "nan1", "fewcomp", "candninf")
EXACT_KINDS = ("exact", "tie64", "tieadj", "tiecut", "ninf")


def _exact_row(K, n, dom=None):
    """One dominant entry; every other one -inf or at least GAP below it (small-integer offsets, distinct ranks)."""
    k = np.arange(K)
    tier = 1 + (3 * k + n) % 3
    row = 3.0 + (n % 5) - GAP * tier - (1 + (7 * k + 2 * n) % 11).astype(np.float64)
    row[(k + n) % 6 == 5] = -np.inf
    row[(5 * n + 3) % K if dom is None else dom] = 3.0 + (n % 5)
    return row


def _generic_row(K, n):
    k = np.arange(K)
    row = 20.0 * np.sin(1.7 * k + 0.37 * n + 0.5) + 1e-3 * k
    assert K == 1 or np.diff(np.sort(row)).min() > 1e-7, "the generic rows are meant to have no ties"
    return row


def _topk_row(kind, K, n, topK, cand_n, masks, moff):
    dom = (5 * n + 3) % K
    if kind == "exact":
        return _exact_row(K, n)
    if kind in ("tie64", "tieadj"):
        row = _exact_row(K, n)
        step = 64 if kind == "tie64" and K > 64 else 1
        a = (dom + 1 + n) % (K - step) if K > step else 0
        if a == dom or a + step == dom:
            a = (a + 2) % max(K - step, 1)
        if K > step and a != dom and a + step != dom:
            row[a] = row[a + step] = row[dom] - GAP          # the two best below the dominant entry
        return row
    if kind == "alleq":
        return np.full(K, 2.5)
    if kind == "tiecut":
        # ranks 1 .. K along a position-dependent permutation, distinct, with ranks topK and topK + 1 equal (the last two
        # when topK == K)
        perm = (np.arange(K) * (2 * (K // 3) + 1 if np.gcd(2 * (K // 3) + 1, K) == 1 else 1) + n) % K
        vals = 3.0 - GAP * (np.arange(K) > 0) - np.arange(K).astype(np.float64)
        cut = min(topK, K - 1)
        if cut >= 1 and K > 2:
            vals[cut] = vals[cut - 1] if cut > 1 else vals[cut]
            if cut == 1:
                vals[2] = vals[1]
        row = np.empty(K)
        row[perm] = vals
        return row
    if kind == "ninf":
        row = np.full(K, -np.inf)
        row[dom] = 1.0
        if K > 2:
            row[(dom + K // 2) % K] = 1.0 - GAP - 2
        return row
    row = _generic_row(K, n)
    if kind == "nan1":
        row[(dom + 1) % K] = np.nan
    elif kind == "fewcomp":
        keep = row.copy()
        row[:] = np.nan
        idx = [(dom + 3 * i) % K for i in range(max(topK - 1, 0))]
        row[idx] = keep[idx]
    elif kind == "candninf":
        j0 = n % len(cand_n)
        row[1 + cand_n[j0]] = -np.inf
        for s, mk in enumerate(masks):
            if (int(mk) >> j0) & 1:
                row[moff + s] = -np.inf
    return row


def _topk_operands(name, topK):
    H, Hp, S, mult, N, _, _, first = TOPK_CASES[name]
    single = mult * H
    K, moff = 1 + single + S, 1 + single
    s = np.arange(S)
    # arbitrary 16-bit patterns (the kernel never sees a state matrix); bit 15 set in every third one
    masks = ((s * 40503 + 12345) & 0x7FFF | np.where(s % 3 == 0, 0x8000, 0)).astype(np.uint16)
    cand = np.stack([((np.arange(Hp) * 7 + 3 * n) % H if np.gcd(7, H) == 1 else (np.arange(Hp) + n) % H) for n in range(N)]).astype(np.int32)
    assert all(len(set(c)) == Hp for c in cand) and cand.min() >= 0 and cand.max() < H
    kinds = [ROW_KINDS[(first + n) % len(ROW_KINDS)] for n in range(N)]
    F = np.stack([_topk_row(kinds[n], K, n, topK, cand[n], masks, moff) for n in range(N)])
    return dict(H=H, Hp=Hp, S=S, single=single, K=K, N=N, masks=masks, cand=cand, F=F, kinds=kinds)


_TOPK_REF = {}


def _topk_ref(name, topK):
    if (name, topK) not in _TOPK_REF:
        c = _topk_operands(name, topK)
        c["ref"] = R.topk(c["F"], c["cand"], c["masks"], c["H"], c["single"], topK)
        _TOPK_REF[(name, topK)] = c
    return _TOPK_REF[(name, topK)]


def _launch_topk(dev, det, c, topK, layout, entry="cols", over=()):
    N, H, Hp, S, K = c["N"], c["H"], c["Hp"], c["S"], c["K"]
    ins = dict(F=EmbX(c["F"], _ld(K, layout, 0), dev), cand=_mat(c["cand"], dev))
    if S:
        ins["masks"] = _vec(c["masks"], dev)
    outs = dict(top_idx=_mat(np.zeros((N, topK), np.int32), dev, fill=False), top_lpc=_mat(np.zeros((N, topK)), dev, fill=False),
                top_rel=_mat(np.zeros((N, topK)), dev, fill=False), marg=EmbX(np.zeros((N, H)), max(_ld(H, layout, 1), H), dev, fill=False))
    a = dict(ldl=ins["F"].ld, N=N, H=H, Hp=Hp, S=S, single=c["single"], topK=topK, ldm=outs["marg"].ld,
             masks=ins["masks"].ptr if S else None)
    a.update(dict(over))
    lib = _lib_of(det)
    tail = (outs["top_idx"].ptr, outs["top_lpc"].ptr, outs["top_rel"].ptr, outs["marg"].ptr, a["ldm"], _stream())
    if entry == "cols":
        rc = lib.pm_infer_topk_cols_f64(ins["F"].ptr, a["ldl"], ins["cand"].ptr, a["masks"], a["N"], a["H"], a["Hp"], a["S"], a["single"],
                                        a["topK"], *tail)
    else:
        rc = lib.pm_infer_topk_f64(ins["F"].ptr, a["ldl"], ins["cand"].ptr, a["masks"], a["N"], a["H"], a["Hp"], a["S"], a["topK"], *tail)
    return rc, outs, ins


def _check_topk(out, c, topK, det, tag):
    ref, kinds = c["ref"], c["kinds"]
    N, H = c["N"], c["H"]
    assert np.array_equal(out["top_idx"], ref["top_idx"]), (tag, "top_idx", np.argwhere(out["top_idx"] != ref["top_idx"])[:6])
    _exact(out["top_rel"], ref["top_rel"], (tag, "top_rel"))
    ex = np.asarray([k in EXACT_KINDS for k in kinds])
    alse = np.abs(np.where(np.isfinite(_f(ref["lse"])), ref["lse"], 0))[:, None]
    with np.errstate(all="ignore"):
        vl = np.where(np.isfinite(_f(ref["top_lpc"])), np.abs(ref["top_lpc"] + ref["lse"][:, None]), 0)
        vm = np.where(np.isfinite(_f(ref["marg"])), np.abs(ref["marg"] + ref["lse"][:, None]), 0)
    _bounded(out["top_lpc"], ref["top_lpc"], RTOL * (1 + alse + vl), "topk", "top_lpc", det, tag)
    _bounded(out["marg"], ref["marg"], RTOL * (1 + alse + vm), "topk", "marg", det, tag)
    is_cand = np.zeros((N, H), bool)
    is_cand[np.arange(N)[:, None], c["cand"]] = True
    _exact(out["top_lpc"], ref["top_lpc"], (tag, "top_lpc of the exact rows"), where=np.broadcast_to(ex[:, None], (N, topK)))
    _exact(out["marg"], ref["marg"], (tag, "marginals of the exact rows"), where=ex[:, None] & (~is_cand | ref["marg_single"]))


@pytest.mark.parametrize("name", list(TOPK_CASES))
def test_infer_topk_cols(dev, name):
    """pm_infer_topk_cols_f64 at K = 2 (S = 0, masks NULL), 63, 64, 65, 129, 200 and the grid-stride case of 16389 rows of three
    columns; topK of 1, 5, K and 70; H' of 1, 4 and 16 with mask bit 15 set; single_cols of H, 2 H and 3 H; ten kinds of rows (exact,
    a tie between columns k and k + 64 -- one lane --, between adjacent columns -- two lanes --, a whole row equal, a tie across the
    topK cut, more -inf entries than K - topK, generic, one NaN, fewer than topK comparable entries, a candidate whose every term is
    -inf).  pm_infer_topk_f64 is called in the cases with single_cols == H and must give the same bits."""
    H, Hp, S, mult, N, topKs, all_layouts, _ = TOPK_CASES[name]
    for topK in topKs:
        c = _topk_ref(name, topK)
        for layout in _two_layouts(all_layouts):
            res = {}
            for det in LIBS:
                for rep in range(2):
                    entry = "plain" if (mult == 1 and rep == 1) else "cols"
                    rc, outs, ins = _launch_topk(dev, det, c, topK, layout, entry)
                    tag = (name, topK, layout, det, entry)
                    _finish(rc, tag, outs, ins)
                    out = res[(det, rep)] = {k: e.host() for k, e in outs.items()}
                    _check_topk(out, c, topK, det, tag)
            _all_equal(res, (name, topK, layout))


def test_infer_topk_row_kinds_are_all_there():
    """Every kind of row occurs at K > 64 (the k / k + 64 pair in one lane) and at K <= 64, and the ties are ties."""
    seen = {}
    for name, spec in TOPK_CASES.items():
        c = _topk_operands(name, spec[5][-1])
        for n, kind in enumerate(c["kinds"]):
            seen.setdefault(kind, set()).add(c["K"] > 64)
            row = c["F"][n]
            if kind == "tie64" and c["K"] > 64:
                order = R.ranking(row)
                assert row[order[1]] == row[order[2]] and abs(order[1] - order[2]) == 64, (name, n)
            if kind == "tieadj" and c["K"] > 3:
                order = R.ranking(row)
                assert row[order[1]] == row[order[2]] and abs(order[1] - order[2]) == 1, (name, n)
    assert all(seen.get(k) == {True, False} for k in ROW_KINDS), seen
    c = _topk_operands("k129", 5)
    row = c["F"][c["kinds"].index("tiecut")]
    order = R.ranking(row)
    assert row[order[4]] == row[order[5]] and row[order[3]] != row[order[4]]


def test_infer_topk_rejects(dev):
    """What the launcher refuses before it launches: the code, and no operand changed."""
    c = _topk_ref("k63", 5)
    for det in LIBS:
        for over, want in ((dict(topK=c["K"] + 1), PM_ERANGE), (dict(ldl=c["K"] - 1), PM_EINVAL), (dict(single=c["H"] - 1), PM_EINVAL),
                           (dict(masks=None), PM_EINVAL), (dict(Hp=17), PM_ERANGE), (dict(ldm=c["H"] - 1), PM_EINVAL),
                           (dict(topK=0), PM_EINVAL)):
            rc, outs, ins = _launch_topk(dev, det, c, 5, "odd", over=over)
            _rejected(rc, want, (over, det), outs, ins)


# ============================================================================================ pm_infer_topk_signed_f64
# name: (S, Hp, H, N, topKs, candidate kind)
SIGNED_CASES = {
    "s3":     (3, 1, 4, 5, (1, 3), "distinct"),
    "s64":    (64, 3, 7, 5, (1, 4, 64), "repeat"),
    "s65":    (65, 5, 7, 5, (1, 4, 65), "distinct"),
    "s65eq":  (65, 3, 7, 1, (4,), "equal"),
    "s130":   (130, 3, 7, 5, (1, 4, 130), "repeat"),
    "s130d":  (130, 5, 9, 5, (4,), "repeat"),
    "s3big":  (3, 1, 2, 16384 + 5, (1, 3), "distinct"),
}
SIGNED_KINDS = ("exact", "tie_in", "tie_cut", "tie_beyond", "generic", "normtie")


def _signed_row(kind, S, n, topK):
    if kind == "generic":
        return _generic_row(S, n)
    dom = (5 * n + 1) % S
    if kind == "normtie":
        # 50.0, then 1.0 and 1.0 + 2^-52, the rest at most 50 - GAP: lse == 50.0 exactly, both differences round to -49.0
        row = 50.0 - GAP - 1.0 - np.arange(S).astype(np.float64)
        row[dom] = 50.0
        if S >= 3:
            row[(dom + 1) % S], row[(dom + 2) % S] = 1.0, 1.0 + 2.0 ** -52
        return row
    # distinct ranks: the dominant entry, then GAP + 1, GAP + 2, ... below it along a permutation
    order = [dom] + [k for k in ((np.arange(S) * 3 + n) % S if S % 3 else (np.arange(S) + n) % S) if k != dom]
    vals = 3.0 - GAP * (np.arange(S) > 0) - np.arange(S).astype(np.float64)
    a = {"tie_in": max(min(topK, S) - 2, 0) if topK > 1 else None, "tie_cut": topK - 1, "tie_beyond": topK + 1}.get(kind)
    if a is not None and a >= 1 and a + 1 < S:
        vals[a + 1] = vals[a]
    row = np.empty(S)
    row[order] = vals
    return row


def _signed_operands(name, topK):
    S, Hp, H, N, _, ckind = SIGNED_CASES[name]
    k, j = np.arange(S)[:, None], np.arange(Hp)[None, :]
    vals = np.array([[-1, 0, 1]], dtype=np.int8).T if S == 3 else (((k * 5 + 2 * j + (k // 3) * j) % 3) - 1).astype(np.int8)
    repeats = {3: [[2, 2, 5], [1, 4, 1]], 5: [[2, 2, 5, 1, 2], [6, 1, 4, 1, 6]]}
    cand = np.empty((N, Hp), np.int32)
    for n in range(N):
        if ckind == "equal":
            cand[n] = (3 + n) % H
        elif ckind == "repeat" and n % 3 != 2:
            cand[n] = repeats[Hp][n % 2]
        else:
            cand[n] = (np.arange(Hp) * 2 + n) % H if H % 2 else (np.arange(Hp) + n) % H
    assert cand.min() >= 0 and cand.max() < H
    kinds = [SIGNED_KINDS[(n + len(name)) % len(SIGNED_KINDS)] for n in range(N)]
    F = np.stack([_signed_row(kinds[n], S, n, topK) for n in range(N)])
    return dict(S=S, Hp=Hp, H=H, N=N, vals=vals, cand=cand, F=F, kinds=kinds)


def _launch_signed(dev, det, c, topK, layout, rank=1, top_idx=None, with_am=True, with_tie=True, over=()):
    N, H, Hp, S = c["N"], c["H"], c["Hp"], c["S"]
    ins = dict(F=EmbX(c["F"], _ld(S, layout, 0), dev), cand=_mat(c["cand"], dev), vals=_mat(c["vals"], dev))
    outs = dict(top_lpc=_mat(np.zeros((N, topK)), dev, fill=False), top_post=_mat(np.zeros((N, topK)), dev, fill=False),
                s=_mat(np.zeros((N, topK * H), np.int8), dev, fill=False), m=_mat(np.zeros((N, H)), dev, fill=False),
                am=_mat(np.zeros((N, H)), dev, fill=False), tie=_vec(np.zeros(N, np.int32), dev, fill=False))
    if rank:
        outs["top_idx"] = _mat(np.zeros((N, topK), np.int32), dev, fill=False)
        tip = outs["top_idx"].ptr
    else:
        ins["top_idx"] = _mat(np.asarray(top_idx, np.int32), dev)
        tip = ins["top_idx"].ptr
    a = dict(ldl=ins["F"].ld, Hp=Hp, S=S, topK=topK, H=H)
    a.update(dict(over))
    rc = _lib_of(det).pm_infer_topk_signed_f64(ins["F"].ptr, a["ldl"], ins["cand"].ptr, ins["vals"].ptr, N, a["H"], a["Hp"], a["S"], a["topK"],
                                                rank, tip, outs["top_lpc"].ptr, outs["top_post"].ptr,
                                                outs["tie"].ptr if with_tie else None, outs["s"].ptr, outs["m"].ptr,
                                                outs["am"].ptr if with_am else None, _stream())
    return rc, outs, ins


def _check_signed(outs, c, ref, topK, rank, with_am, with_tie, det, tag):
    N, H, S = c["N"], c["H"], c["S"]
    if rank:
        got = outs["top_idx"].host()
        assert np.array_equal(got, ref["top_idx"]), (tag, "top_idx", np.argwhere(got != ref["top_idx"])[:6])
        assert np.array_equal(outs["tie"].host()[0], ref["tie"]), (tag, "tie", outs["tie"].host()[0][:12], ref["tie"][:12])
    else:
        assert outs["tie"].unchanged(), (tag, "tie was written with rank == 0")
    if not with_tie:
        assert outs["tie"].unchanged(), (tag, "tie is NULL")
    alse = np.abs(_f(ref["lse"]))[:, None]
    with np.errstate(all="ignore"):
        vl = np.where(np.isfinite(_f(ref["top_lpc"])), np.abs(ref["top_lpc"] + ref["lse"][:, None]), 0)
    _bounded(outs["top_lpc"].host(), ref["top_lpc"], RTOL * (1 + alse + vl), "signed", "top_lpc", det, tag)
    _bounded(outs["top_post"].host(), ref["top_post"], RTOL * (1 + alse + vl), "signed", "top_post", det, tag)
    # s: the written entries equal the reference's, every other one still holds the pattern
    s = outs["s"].host().reshape(N, topK, H)
    assert np.array_equal(s[ref["s_written"]], ref["s"][ref["s_written"]]), (tag, "s_out")
    assert (s[~ref["s_written"]] == SENT_I8).all(), (tag, "an entry of s_out outside the candidates (or of an invalid index) was written")
    for k, want in (("m", ref["m"]), ("am", ref["am"])):
        got = outs[k].host()
        if k == "am" and not with_am:
            assert outs[k].unchanged(), (tag, "am_out is NULL: nothing else may be written")
            continue
        w = ref["m_written"]
        assert (_bits(got)[~w] == _bits(np.array([PATTERN]))[0]).all(), (tag, k, "an entry of another latent was written")
        _bounded(got[w], want[w], RTOL * ref["am_mag"][w] + FLOOR, "signed", k, det, tag)
    # exact-class rows: the dominant state has posterior exactly 1, so its non-zero positions get exactly +-1 / 1 -- at the
    # position that wins each latent
    m_host, am_host = outs["m"].host(), outs["am"].host()
    for n in range(N):
        if c["kinds"][n] in ("generic",):
            continue
        dom = int(np.argmax(c["F"][n]))
        last = {int(cc): j for j, cc in enumerate(c["cand"][n])}
        for cc, j in last.items():
            v = int(c["vals"][dom, j])
            if v:
                assert m_host[n, cc] == float(v), (tag, n, cc, "m of the dominant state's position")
                assert not with_am or am_host[n, cc] == 1.0, (tag, n, cc, "am of the dominant state's position")


@pytest.mark.parametrize("name", list(SIGNED_CASES))
def test_infer_topk_signed(dev, name):
    """pm_infer_topk_signed_f64 with rank != 0 at S = 3, 64, 65, 130 and 16389 rows of S = 3, topK of 1, 4 and S, H' of 1, 3, 5;
    candidates distinct, repeated ([2, 2, 5], [1, 4, 1]: the last position wins) and all equal; s_out, m_out and am_out start as
    the pattern, so "left as they are" is checked entry by entry; am_out given and NULL.  The tie flag to equality on rows with
    an exact tie inside topK, across the cut, beyond topK + 1 only (flag 0), none, and a tie of the normalised values only."""
    S, Hp, H, N, topKs, _ = SIGNED_CASES[name]
    for topK in topKs:
        c = _signed_operands(name, topK)
        ref = R.topk_signed(c["F"], c["cand"], c["vals"], H, topK, 1)
        want_ties = {k: int(ref["tie"][n]) for n, k in enumerate(c["kinds"])}
        if S >= topK + 3 and topK >= 3:
            assert want_ties.get("tie_in", 1) == 1 and want_ties.get("tie_cut", 1) == 1 and want_ties.get("tie_beyond", 0) == 0 \
                and want_ties.get("generic", 0) == 0 and want_ties.get("normtie", 1) == 1, (name, topK, want_ties)
        for layout in _two_layouts(name == "s65"):
            res = {}
            for det in LIBS:
                for rep in range(2):
                    with_am = rep == 0
                    rc, outs, ins = _launch_signed(dev, det, c, topK, layout, with_am=with_am)
                    tag = (name, topK, layout, det, with_am)
                    _finish(rc, tag, outs, ins, unwritten=("s", "m", "am"))
                    _check_signed(outs, c, ref, topK, 1, with_am, True, det, tag)
                    res[(det, rep)] = {k: e.host() for k, e in outs.items() if k != "am"}
            _all_equal(res, (name, topK, layout))


@pytest.mark.parametrize("name", ["s64", "s130"])
def test_infer_topk_signed_given_indices(dev, name):
    """rank == 0: top_idx is an input -- a permutation that is not the device's order, an index -1 and an index S (both give
    -inf / 0 and leave their s_out row as it is); tie is not written, and may be NULL."""
    S, Hp, H, N, _, _ = SIGNED_CASES[name]
    topK = 4
    c = _signed_operands(name, topK)
    ranked = R.topk_signed(c["F"], c["cand"], c["vals"], H, topK, 1)["top_idx"]
    given = ranked[:, ::-1].copy()
    given[0, 1], given[1, 0], given[2, 3] = -1, S, (ranked[2, 0] + 7) % S
    assert not np.array_equal(given, ranked)
    ref = R.topk_signed(c["F"], c["cand"], c["vals"], H, topK, 0, given)
    res = {}
    for det in LIBS:
        for rep in range(2):
            rc, outs, ins = _launch_signed(dev, det, c, topK, "odd", rank=0, top_idx=given, with_tie=rep == 0)
            tag = (name, det, rep)
            _finish(rc, tag, outs, ins, unwritten=("s", "m", "am", "tie"))
            _check_signed(outs, c, ref, topK, 0, True, rep == 0, det, tag)
            res[(det, rep)] = {k: e.host() for k, e in outs.items()}
    _all_equal(res, name)


def test_infer_topk_signed_rejects(dev):
    c = _signed_operands("s64", 4)
    for det in LIBS:
        for over, kw, want in ((dict(topK=65), {}, PM_ERANGE), (dict(ldl=63), {}, PM_EINVAL), (dict(Hp=17), {}, PM_ERANGE),
                               ({}, dict(with_tie=False), PM_EINVAL), (dict(S=0), {}, PM_EINVAL)):
            rc, outs, ins = _launch_signed(dev, det, c, 4, "odd", over=over, **kw)
            _rejected(rc, want, (over, kw, det), outs, ins)


# ======================================================================================================== k-th select
def _kth_data(name):
    """Keys (uint64) built bit by bit so that the scan's seams are hit on purpose, and the ranks k to ask for."""
    rng = np.random.RandomState(len(name) + 11)
    if name == "lowbits":                      # values differing only in bits [0, 4): rounds 0-4 see one bin
        keys = np.uint64(0xC05A3B1C2D4E6F70) | rng.randint(0, 16, size=300).astype(np.uint64)
    elif name == "alleq":
        keys = np.full(257, 0xBFF123456789ABCD, dtype=np.uint64)
    elif name in ("digits0", "digits1"):       # chosen digits at 0, 15, 16, 4095 and 16 q +- 1, in the first / second round
        ds = np.array([0, 15, 16, 4095, 16 * 7 - 1, 16 * 7, 16 * 7 + 1, 16 * 255 - 1, 16 * 255, 16 * 200 + 15, 16 * 201], dtype=np.uint64)
        d = ds[rng.randint(0, len(ds), size=330)]
        low = rng.randint(0, 1 << 20, size=330).astype(np.uint64) << np.uint64(11)
        keys = (d << np.uint64(52)) | low if name == "digits0" else (np.uint64(0xC01) << np.uint64(52)) | (d << np.uint64(40)) | low
    elif name == "specials":
        x = np.concatenate([rng.normal(size=200) * 50, [np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 3.5, 3.5]])
        keys = np.concatenate([R.keys_of(x), R.keys_of(np.array([0x7FF8000000000001, 0xFFF8000000000001], dtype=np.uint64).view(np.float64))])
    else:                                      # "big": 262144 + 300 values -- the grid-stride loop of both histogram kernels
        x = np.concatenate([rng.normal(size=262144 + 290) * 50 - 600.0, [np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 1e-310, 3.5, 3.5, -1e-310]])
        keys = R.keys_of(x)
    rng.shuffle(keys)
    n = len(keys)
    ks = {1, 2, n // 2, n - 1, n}
    if name != "big":
        # cumulative counts from the top at every distinct first / second digit: above + bin == k, and k - 1
        for shift in (52, 40):
            dig = np.sort((keys >> np.uint64(shift)).astype(np.uint64))[::-1]
            edges = np.flatnonzero(np.diff(dig.astype(np.float64)) != 0) + 1
            for e in edges[:4].tolist() + edges[-2:].tolist():
                ks.update({int(e), int(e) + 1})
        ks.add(n + 3)                          # past the end: "chunk 0 if none" of the scan
    return keys, sorted(k for k in ks if k >= 1)


def _kth_protocol_a(dev, lib, shards, k, ref_states, ref_hists, tag):
    """pm_kth_hist_f64 / pm_kth_scan / pm_kth_value_f64: the shards histogram into one table (what the all-reduce amounts to)."""
    st = _vec(np.array([0, k], dtype=np.uint64), dev)
    hist = _vec(np.zeros(R.BINS, dtype=np.uint64), dev)
    out = _vec(np.zeros(1), dev, fill=False)
    for r, (shift, bits) in enumerate(R.KTH_ROUNDS):
        for sh in shards:
            x, n = (sh.ptr, sh.n) if sh.n else (None, 0)
            rc = lib.pm_kth_hist_f64(x, n, st.ptr, shift, bits, hist.ptr, _stream())
            assert rc == PM_OK, (tag, r, rc)
        torch.cuda.synchronize()
        assert np.array_equal(hist.host()[0], ref_hists[r]), (tag, "histogram of round", r)
        assert np.array_equal(st.host()[0], ref_states[r]), (tag, "pm_kth_hist_f64 wrote the state", r)
        assert lib.pm_kth_scan(hist.ptr, st.ptr, shift, bits, _stream()) == PM_OK
        torch.cuda.synchronize()
        assert np.array_equal(st.host()[0], ref_states[r + 1]), (tag, "state after round", r, st.host()[0], ref_states[r + 1])
        assert not hist.host().any(), (tag, "the scan leaves the histogram cleared")
    assert lib.pm_kth_value_f64(st.ptr, out.ptr, _stream()) == PM_OK
    torch.cuda.synchronize()
    assert st.outside_untouched() and hist.outside_untouched() and out.outside_untouched() and all(s.unchanged() for s in shards), tag
    return out.host()[0].view(np.uint64)[0]


def _kth_protocol_b(dev, lib, shards, k, ref_states, ref_hists, tag, k0_arg, rezero, bufs=None):
    """pm_kth_round_f64 / pm_kth_final_f64 (or _k / _z): one (states, hists) pair per 'rank', summed by hand between rounds."""
    fresh = bufs is None
    if fresh:
        bufs = []
        for _ in shards:
            states = np.zeros(14, dtype=np.uint64)
            states[1] = k
            # (the rank as an argument: slot 0 is deliberately left holding the pattern)
            bufs.append((_vec(states, dev, fill=not k0_arg), _vec(np.zeros(6 * R.BINS, dtype=np.uint64), dev)))
    prev = (0, 1)

    def allreduce(r):
        tot = sum(h.block().view(6, R.BINS)[r].clone() for _, h in bufs)
        for _, h in bufs:
            h.block().view(6, R.BINS)[r] = tot
        return tot.cpu().numpy().view(np.uint64)

    for r, (shift, bits) in enumerate(R.KTH_ROUNDS):
        if r:
            assert np.array_equal(allreduce(r - 1), ref_hists[r - 1]), (tag, "histogram of round", r - 1)
        for sh, (st, hs) in zip(shards, bufs):
            x, n = (sh.ptr, sh.n) if sh.n else (None, 0)
            if k0_arg:
                rc = lib.pm_kth_round_k_f64(x, n, st.ptr, hs.ptr, r, prev[0], prev[1], shift, bits, k if r == 0 else -1, _stream())
            else:
                rc = lib.pm_kth_round_f64(x, n, st.ptr, hs.ptr, r, prev[0], prev[1], shift, bits, _stream())
            assert rc == PM_OK, (tag, r, rc)
        torch.cuda.synchronize()
        for st, _ in bufs:
            got = st.host()[0].reshape(7, 2)
            assert np.array_equal(got[:r + 1], ref_states[:r + 1]), (tag, "states after the launch of round", r, got[:r + 1], ref_states[:r + 1])
            if fresh:          # the slots of the rounds to come: still zero, or still the pattern
                assert (got[r + 1:] == (SENT_I64 if k0_arg else 0)).all(), (tag, "a state slot past round", r, "was written")
        prev = (shift, bits)
    assert np.array_equal(allreduce(5), ref_hists[5]), (tag, "histogram of round 5")
    values = []
    for st, hs in bufs:
        out = _vec(np.zeros(1), dev, fill=False)
        if rezero is None:
            rc = lib.pm_kth_final_f64(st.ptr, hs.ptr, 6, prev[0], prev[1], out.ptr, _stream())
        else:
            rc = lib.pm_kth_final_z_f64(st.ptr, hs.ptr, 6, prev[0], prev[1], out.ptr, int(rezero), _stream())
        torch.cuda.synchronize()
        assert rc == PM_OK and out.outside_untouched() and st.outside_untouched() and hs.outside_untouched(), tag
        assert np.array_equal(st.host()[0].reshape(7, 2), ref_states), (tag, "the seven states", st.host()[0].reshape(7, 2), ref_states)
        if rezero:
            assert not hs.host().any(), (tag, "rezero = 1 leaves all six histograms zero")
        else:
            assert np.array_equal(hs.host()[0].reshape(6, R.BINS), ref_hists), (tag, "the histograms are left intact")
        values.append(out.host()[0].view(np.uint64)[0])
    assert all(s.unchanged() for s in shards), tag
    return values, bufs


class _Shard(EmbX):
    def __init__(self, x, dev):
        x = np.asarray(x, dtype=np.float64)
        self.n = len(x)
        super().__init__(x if self.n else np.zeros(1), max(self.n, 1), dev)


@pytest.mark.parametrize("name", ["lowbits", "alleq", "digits0", "digits1", "specials", "big"])
def test_kth_select(dev, name):
    """Both protocols -- pm_kth_hist_f64 / pm_kth_scan / pm_kth_value_f64 and pm_kth_round(_k)_f64 / pm_kth_final(_z)_f64 -- over
    two 'ranks' (split in two, and an EMPTY shard with a NULL pointer beside the full one), every round's state and histogram
    against the reference's, the value bit for bit.  Keys differing only in bits [0, 4); all equal; chosen digits at 0, 15, 16,
    4095 and 16 q +- 1 in the first and in the second round with k on the cumulative counts (above + bin == k and k - 1) and past
    the end; +-inf, +-0, denormals and two NaNs of opposite sign; 262444 values for the grid-stride loops."""
    keys, ks = _kth_data(name)
    x = R.doubles_of_keys(keys)
    assert np.array_equal(R.keys_of(x), keys)
    cut = len(x) // 3
    splits = [[_Shard(x[:cut], dev), _Shard(x[cut:], dev)], [_Shard(x[:0], dev), _Shard(x, dev)]]
    by_rank = np.sort(keys)
    for k in ks:
        want, ref_states, ref_hists = R.kth([keys], k)
        if k <= len(keys):
            assert R.key_of_int(want) == int(by_rank[-k]), (name, k, "the reference against a full sort")
        res = {}
        for det in LIBS:
            lib = _lib_of(det)
            for rep in range(2):
                tag = (name, k, det, rep)
                a = _kth_protocol_a(dev, lib, splits[rep], k, ref_states, ref_hists, tag)
                vals, _ = _kth_protocol_b(dev, lib, splits[rep], k, ref_states, ref_hists, tag, k0_arg=rep == 1, rezero=None if rep == 0 else 0)
                assert a == want and all(v == want for v in vals), (tag, hex(int(a)), [hex(int(v)) for v in vals], hex(int(want)))
                res[(det, rep)] = dict(a=np.array([a]), b=np.array(vals))
        _all_equal(res, (name, k))


def test_kth_rezero_and_second_select(dev):
    """pm_kth_round_k_f64 + pm_kth_final_z_f64 with rezero = 1: the six histograms are left zero, and a second select on the same
    buffers WITHOUT any fill -- states still holding the first select's seven pairs -- gives the right value."""
    keys, _ = _kth_data("digits1")
    x = R.doubles_of_keys(keys)
    for det in LIBS:
        lib = _lib_of(det)
        shards = [_Shard(x[:100], dev), _Shard(x[100:], dev)]
        bufs = None
        for k in (len(x) // 2, 3, len(x)):
            want, ref_states, ref_hists = R.kth([keys], k)
            vals, bufs = _kth_protocol_b(dev, lib, shards, k, ref_states, ref_hists, ("second select", k, det), k0_arg=True, rezero=1, bufs=bufs)
            assert all(v == want for v in vals), (k, det)


def test_kth_rejects(dev):
    """bits = 13, shift + bits > 64, round = 6, k0 >= 0 with round > 0: refused before any launch."""
    x = _Shard(np.arange(10.0), dev)
    st, hs, out = _vec(np.zeros(14, np.uint64), dev), _vec(np.zeros(6 * R.BINS, np.uint64), dev), _vec(np.zeros(1), dev)
    ops = dict(x=x, st=st, hs=hs, out=out)
    for det in LIBS:
        lib = _lib_of(det)
        s = _stream()
        for rc in (lib.pm_kth_hist_f64(x.ptr, 10, st.ptr, 40, 13, hs.ptr, s), lib.pm_kth_hist_f64(x.ptr, 10, st.ptr, 56, 12, hs.ptr, s),
                   lib.pm_kth_scan(hs.ptr, st.ptr, 40, 13, s), lib.pm_kth_scan(hs.ptr, st.ptr, 60, 5, s),
                   lib.pm_kth_round_f64(x.ptr, 10, st.ptr, hs.ptr, 6, 4, 12, 0, 4, s),
                   lib.pm_kth_round_f64(x.ptr, 10, st.ptr, hs.ptr, 0, 0, 1, 40, 13, s),
                   lib.pm_kth_round_f64(x.ptr, 10, st.ptr, hs.ptr, 1, 52, 12, 53, 12, s),
                   lib.pm_kth_round_k_f64(x.ptr, 10, st.ptr, hs.ptr, 1, 52, 12, 40, 12, 3, s),
                   lib.pm_kth_round_k_f64(x.ptr, 10, st.ptr, hs.ptr, 6, 4, 12, 0, 4, -1, s),
                   lib.pm_kth_final_z_f64(st.ptr, hs.ptr, 7, 0, 4, out.ptr, 1, s), lib.pm_kth_final_f64(st.ptr, hs.ptr, 6, 60, 5, out.ptr, s),
                   lib.pm_kth_value_f64(None, out.ptr, s)):
            _rejected(rc, PM_EINVAL, det, ops, {})


# ================================================================================================== inverse kernels
def _pack(mats, ld, stride, n):
    """Matrices (batch, n, n) at b * stride + i * ld + j of a flat buffer whose every other element holds the pattern."""
    batch = len(mats)
    flat = np.full((batch - 1) * stride + (n - 1) * ld + n, PATTERN)
    used = np.zeros(len(flat), bool)
    idx = (np.arange(batch)[:, None, None] * stride + np.arange(n)[None, :, None] * ld + np.arange(n)[None, None, :])
    flat[idx] = np.asarray(mats)
    used[idx] = True
    return flat, used, idx


def _unpack(e, used, idx, tag, written=True):
    flat = e.host()[0]
    assert (_bits(flat)[~used] == _bits(np.array([PATTERN]))[0]).all(), (tag, "an element between the rows or the matrices was written")
    assert e.outside_untouched(), (tag, "a guard element was written")
    if written:
        assert (_bits(flat)[used] != _bits(np.array([PATTERN]))[0]).all(), (tag, "an element of the result was not written")
    return flat[idx]


def _spd(n, seed, rel=0.0):
    rs = np.random.RandomState(seed)
    B = rs.normal(size=(n, 3 * n + 5))
    A = B @ B.T
    dadd = rs.uniform(0.1, 1.0, size=n)
    B0 = B + rel * rs.normal(size=B.shape)
    X0 = np.linalg.inv(B0 @ B0.T + np.diag(dadd))
    return A, dadd, 0.5 * (X0 + X0.T)


def _upper_with_junk(A):
    """The upper triangle; the strict lower triangle holds the pattern (never read)."""
    U = np.array(A, dtype=np.float64)
    U[np.tril_indices(len(U), -1)] = PATTERN
    return U


def _sweep(dev, det, mats, dadds, n, layout, batch_entry, with_full=True, ldo_pad=True):
    """pm_spd_inverse_f64 (one matrix) or pm_spd_inverse_batch_f64 on packed, padded operands."""
    batch = len(mats)
    ldu = _ld(n, layout, 0) if layout != "tight" else n
    ldo = (_ld(n, layout, 1) if layout != "tight" else n) if ldo_pad else n
    s_in, s_out = ldu * (n - 1) + n + (0 if layout == "tight" else 5), ldo * (n - 1) + n + (0 if layout == "tight" else 3)
    fin, _, _ = _pack([_upper_with_junk(m) for m in mats], ldu, s_in, n)
    ins = dict(upper=_vec(fin, dev))
    if dadds is not None:
        ins["dadd"] = _vec(np.concatenate(dadds), dev)
    oflat, used, idx = _pack(np.zeros((batch, n, n)), ldo, s_out, n)
    outs = dict(inv=_vec(oflat, dev, fill=False), full=_vec(oflat, dev, fill=False), piv=_vec(np.zeros(2 * batch), dev, fill=False))
    lib = _lib_of(det)
    da = ins["dadd"].ptr if dadds is not None else None
    fp = outs["full"].ptr if with_full else None
    if batch_entry:
        rc = lib.pm_spd_inverse_batch_f64(ins["upper"].ptr, ldu, s_in, da, n, fp, outs["inv"].ptr, ldo, s_out, outs["piv"].ptr, batch, _stream())
    else:
        rc = lib.pm_spd_inverse_f64(ins["upper"].ptr, ldu, da, n, fp, outs["inv"].ptr, ldo, outs["piv"].ptr, _stream())
    tag = ("sweep", n, layout, det, batch_entry, with_full, dadds is not None)
    torch.cuda.synchronize()
    assert rc == PM_OK, (tag, rc)
    assert all(e.unchanged() for e in ins.values()), (tag, "an input was written")
    inv = _unpack(outs["inv"], used, idx, tag)
    if with_full:
        full = _unpack(outs["full"], used, idx, tag)
    else:
        assert outs["full"].unchanged(), (tag, "full is NULL")
        full = None
    assert outs["piv"].outside_untouched() and outs["piv"].written(), tag
    return dict(inv=inv, piv=outs["piv"].host()[0].reshape(batch, 2), **({"full": full} if with_full else {}))


def _check_sweep(out, b, Af, det, tag):
    got = out["inv"][b]
    assert np.array_equal(got, got.T), (tag, "inv is not symmetric")
    ref, cond = np.linalg.inv(Af), np.linalg.cond(Af)
    _bounded(got, ref, np.full(got.shape, 1e-14 * cond * np.abs(ref).max()), "sweep", "inv", det, tag)
    d2 = np.diag(np.linalg.cholesky(Af)) ** 2
    want = np.asarray([d2.min(), d2.max()])
    _bounded(out["piv"][b], want, 1e-9 * want, "sweep", "pivots", det, tag)
    if "full" in out:
        assert np.array_equal(out["full"][b], Af), (tag, "full")


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 65, 255])
def test_spd_inverse_layouts(dev, n):
    """pm_spd_inverse_f64 and pm_spd_inverse_batch_f64 (two matrices) with ldu > n, ldo > n and padded batch strides, `full` given
    and NULL, diag_add given and NULL, the pattern in the strict lower triangle: n around the 32-row residue classes."""
    A0, d0, _ = _spd(n, n)
    A1, d1, _ = _spd(n, n + 1000)
    for layout in (LAYOUTS if n == 33 else ("tight", "odd")):
        for with_da in (True, False):
            mats = [A0 if with_da else A0 + np.diag(d0), A1 if with_da else A1 + np.diag(d1)]
            res = {}
            for det in LIBS:
                for rep in range(2):
                    one = _sweep(dev, det, mats[:1], [d0] if with_da else None, n, layout, False, with_full=rep == 0)
                    two = _sweep(dev, det, mats, [d0, d1] if with_da else None, n, layout, True, with_full=rep == 1)
                    tag = (n, layout, with_da, det, rep)
                    _check_sweep(one, 0, A0 + np.diag(d0), det, tag)
                    _check_sweep(two, 0, A0 + np.diag(d0), det, tag)
                    _check_sweep(two, 1, A1 + np.diag(d1), det, tag)
                    assert _same_bits(one["inv"][0], two["inv"][0]) and _same_bits(one["piv"][0], two["piv"][0]), (tag, "batch against single")
                    res[(det, rep)] = dict(inv=two["inv"], piv=two["piv"])
            _all_equal(res, (n, layout, with_da))


def _warm(dev, det, entry, mats, dadds, prevs, n, layout, general_mask=0):
    """The four warm entries.  `full`, `inv` (ldo = n), `prev_inv` (ldp = n) are dense for the single entries; the batch entries
    take padded stride_in / stride_prev / stride_out; `work` is exactly pm_spd_inverse_warm_work_len(n) per matrix."""
    batch = len(mats)
    lib = _lib_of(det)
    single = entry in ("warm", "long")
    pad = layout != "tight"
    ldu = _ld(n, layout, 0) if pad else n
    s_in = ldu * (n - 1) + n + (5 if pad else 0)
    s_prev, s_out = (n * n + (7 if pad else 0), n * n + (3 if pad else 0)) if not single else (n * n, n * n)
    gen = [(general_mask >> b) & 1 for b in range(batch)]
    fin, _, _ = _pack([m if g else _upper_with_junk(m) for m, g in zip(mats, gen)], ldu, s_in, n)
    pin, _, _ = _pack(prevs, n, s_prev, n)
    ins = dict(upper=_vec(fin, dev), prev=_vec(pin, dev))
    if dadds is not None:
        ins["dadd"] = _vec(np.concatenate(dadds), dev)
    oflat, used, idx = _pack(np.zeros((batch, n, n)), n, s_out, n)
    wl = int(lib.pm_spd_inverse_warm_work_len(n))
    tiles = (n + 15) // 16
    assert wl == 6 * n * n + 2 * tiles * tiles + tiles * n + 1
    outs = dict(inv=_vec(oflat, dev, fill=False), work=_vec(np.zeros(batch * wl), dev, fill=False),
                piv=_vec(np.zeros(3 if single else 2 * batch), dev, fill=False), full=_vec(np.zeros(n * n), dev, fill=False),
                acc=_vec(np.zeros(batch), dev, fill=False))
    da = ins["dadd"].ptr if dadds is not None else None
    if single:
        fn = lib.pm_spd_inverse_warm_f64 if entry == "warm" else lib.pm_spd_inverse_warm_long_f64
        rc = fn(ins["upper"].ptr, ldu, da, n, ins["prev"].ptr, n, outs["work"].ptr, outs["full"].ptr, outs["inv"].ptr, n, outs["piv"].ptr, _stream())
    elif entry == "batch":
        rc = lib.pm_spd_inverse_warm_batch_f64(ins["upper"].ptr, ldu, s_in, da, n, ins["prev"].ptr, s_prev, outs["work"].ptr, outs["inv"].ptr,
                                               s_out, outs["piv"].ptr, batch, _stream())
    else:
        rc = lib.pm_inverse_warm_batch_f64(ins["upper"].ptr, ldu, s_in, da, n, ins["prev"].ptr, s_prev, outs["work"].ptr, outs["inv"].ptr,
                                           s_out, outs["piv"].ptr, outs["acc"].ptr, batch, general_mask, _stream())
    tag = (entry, n, layout, det, dadds is not None, general_mask)
    torch.cuda.synchronize()
    assert rc == PM_OK, (tag, rc)
    assert all(e.unchanged() for e in ins.values()), (tag, "an input was written")
    inv = _unpack(outs["inv"], used, idx, tag)
    assert outs["work"].outside_untouched() and outs["piv"].outside_untouched() and outs["piv"].written(), (tag, "work / pivots")
    piv = outs["piv"].host()[0]
    out = dict(inv=inv)
    if single:
        assert outs["full"].outside_untouched() and outs["full"].written(), tag
        out["full"] = outs["full"].host()[0].reshape(1, n, n)
        out["acc"], out["piv"] = piv[2:3].copy(), piv[:2].reshape(1, 2)
        assert outs["acc"].unchanged()
    else:
        assert outs["full"].unchanged(), tag
        out["piv"] = piv.reshape(batch, 2)
        if entry == "batch":
            assert outs["acc"].unchanged()
            out["acc"] = outs["work"].host()[0].reshape(batch, wl)[:, -1].copy()          # the last word of each share
        else:
            assert outs["acc"].outside_untouched() and outs["acc"].written(), tag
            out["acc"] = outs["acc"].host()[0]
    return out


def _check_warm(out, b, Af, X0, det, entry, tag, general=False):
    """The accept / reject logic of tests/test_bsc_gpu.py::test_spd_inverse_warm (and ..._warm_long for the long entry)."""
    n = len(Af)
    got, pv, acc = out["inv"][b], out["piv"][b], float(out["acc"][b])
    At = Af.T if general else Af
    ref, cond = np.linalg.inv(At), np.linalg.cond(Af)
    if not general:
        assert np.array_equal(got, got.T), (tag, "inv is not symmetric")
    if entry == "long":
        _bounded(got, ref, np.full(got.shape, 1e-13 * cond * np.abs(ref).max()), "warm_long", "inv", det, tag)
        assert acc in (1.0, 2.0), (tag, acc)
        return
    R0 = np.eye(n) - (X0 @ At if general else Af @ X0)
    r0 = np.linalg.norm(R0)
    with np.errstate(all="ignore"):
        r3 = np.linalg.norm(np.linalg.matrix_power(R0, 8))
    assert r3 < 0.3e-8, (tag, "the case is meant to be a close start", r3)
    assert acc == (1.0 if r0 < 0.999 else 2.0) or (general and acc == 1.0), (tag, acc, r0)
    _bounded(got, ref, np.full(got.shape, 1e-14 * cond * np.abs(ref).max()), "warm", "inv", det, tag)
    if not general:
        d2 = np.diag(np.linalg.cholesky(Af)) ** 2
        want = np.asarray([1.0 / np.diag(ref).max(), np.diag(Af).max()])
        _bounded(pv, want, 1e-7 * want, "warm", "pivots", det, tag)
        assert pv[0] <= d2.min() * (1 + 1e-7) and pv[1] >= d2.max() * (1 - 1e-12), tag
        assert np.linalg.norm(np.eye(n) - Af @ got) < max(2.0 * r3 ** 2, 1e-11 * cond), tag


@pytest.mark.parametrize("n", [15, 16, 17, 31, 47, 48, 49, 255])
def test_spd_inverse_warm_layouts(dev, n):
    """pm_spd_inverse_warm_f64, pm_spd_inverse_warm_long_f64, pm_spd_inverse_warm_batch_f64 and pm_inverse_warm_batch_f64 from a
    close start (rel = 1e-3) at n around the 16 x 16 tiles of the Newton-Schulz kernels, with padded ldu, stride_in, stride_prev and
    stride_out; `work` exactly pm_spd_inverse_warm_work_len(n) per matrix inside guards; diag_add given and NULL."""
    A0, d0, X0 = _spd(n, n, rel=1e-3)
    A1, d1, X1 = _spd(n, n + 1000, rel=1e-3)
    fulls = [A0 + np.diag(d0), A1 + np.diag(d1)]
    for layout in (LAYOUTS if n == 17 else ("tight", "odd")):
        for with_da in (True, False):
            mats = [A0, A1] if with_da else fulls
            das = [d0, d1] if with_da else None
            res = {}
            for det in LIBS:
                for rep in range(2):
                    tag = (n, layout, with_da, det, rep)
                    r = {}
                    for entry in ("warm", "long"):
                        o = r[entry] = _warm(dev, det, entry, mats[:1], das[:1] if das else None, [X0], n, layout)
                        assert np.array_equal(o["full"][0], fulls[0]), (tag, entry, "full")
                        _check_warm(o, 0, fulls[0], X0, det, entry, tag + (entry,))
                    o = r["batch"] = _warm(dev, det, "batch", mats, das, [X0, X1], n, layout)
                    g = r["general"] = _warm(dev, det, "general", mats, das, [X0, X1], n, layout, general_mask=0)
                    for b in range(2):
                        _check_warm(o, b, fulls[b], [X0, X1][b], det, "batch", tag + ("batch", b))
                        _check_warm(g, b, fulls[b], [X0, X1][b], det, "general", tag + ("mask 0", b))
                    assert _same_bits(o["inv"], g["inv"]) and _same_bits(o["piv"], g["piv"]) and _same_bits(o["acc"], g["acc"]), (tag, "mask 0")
                    assert _same_bits(o["inv"][0], r["warm"]["inv"][0]), (tag, "the batch entry against the single one")
                    res[(det, rep)] = {e + k: v[k] for e, v in r.items() for k in ("inv", "piv", "acc")}
            _all_equal(res, (n, layout, with_da))


@pytest.mark.parametrize("n", [17, 48])
def test_inverse_warm_general_masks(dev, n):
    """pm_inverse_warm_batch_f64 with general_mask = 1 (a GENERAL matrix, given in full, in slot 0 of two), 0b101 on a batch of
    three, and 0: a general matrix comes back as the inverse of its TRANSPOSE, not symmetrised; a symmetric one as from
    pm_spd_inverse_warm_batch_f64, bit for bit."""
    rs = np.random.RandomState(n)
    sym, gens, dadds, prevs_s, prevs_g = [], [], [], [], []
    for b in range(3):
        A, d, X = _spd(n, 10 * n + b, rel=1e-3)
        E = rs.normal(size=(n, n))
        G = A / n + np.diag(d) + 1e-4 * np.abs(A / n).max() * (E - E.T)                 # non-symmetric, diag_add still added
        sym.append(A), dadds.append(d), prevs_s.append(X), gens.append(G - np.diag(d))
        prevs_g.append(np.linalg.inv((G * (1 + 1e-3 * rs.normal(size=(n, n)) / n)).T))
    for mask, batch in ((1, 2), (0b101, 3), (0, 3)):
        mats = [gens[b] if (mask >> b) & 1 else sym[b] for b in range(batch)]
        prevs = [prevs_g[b] if (mask >> b) & 1 else prevs_s[b] for b in range(batch)]
        res = {}
        for layout in ("tight", "odd"):
            for det in LIBS:
                for rep in range(2):
                    o = _warm(dev, det, "general", mats, dadds[:batch], prevs, n, layout, general_mask=mask)
                    plain = _warm(dev, det, "batch", sym[:batch], dadds[:batch], prevs_s[:batch], n, layout)
                    for b in range(batch):
                        tag = (n, mask, b, layout, det)
                        if (mask >> b) & 1:
                            G = gens[b] + np.diag(dadds[b])
                            _check_warm(o, b, G, prevs[b], det, "general", tag, general=True)
                            ref = np.linalg.inv(G)
                            assert np.abs(o["inv"][b] - o["inv"][b].T).max() > 0.1 * np.abs(ref - ref.T).max(), (tag, "symmetrised")
                        else:
                            _check_warm(o, b, sym[b] + np.diag(dadds[b]), prevs[b], det, "general", tag)
                            assert _same_bits(o["inv"][b], plain["inv"][b]) and _same_bits(o["piv"][b], plain["piv"][b]), tag
                    res[(layout, det, rep)] = dict(inv=o["inv"], acc=o["acc"])
        _all_equal(res, (n, mask))


@pytest.mark.parametrize("n", [33, 65, 255])
def test_spd_inverse_exact_case(dev, n):
    """A = L D L^T with dyadic entries (tests/test_select_kernels_cpu.py: every intermediate of the sweep is a float64): `inv`
    and `full` to equality, pivots == [min D, max D] exactly, from the cold entries on padded operands; and on the four warm
    entries with prev_inv = A^-1 exactly: `inv` bit for bit, accepted == 1, pivots[1] == max A_ii, pivots[0] within 1e-7 of
    1 / max X_ii."""
    c = R.spd_exact_case(n, n)
    A, X, d = c["A"], c["X"], c["d"]
    dadd = 0.125 * (1 + np.arange(n) % 3)
    U = A - np.diag(dadd)
    assert np.array_equal(U + np.diag(dadd), A)
    res = {}
    for det in LIBS:
        for rep, layout in enumerate(("tight", "odd")):
            tag = (n, det, layout)
            one = _sweep(dev, det, [U], [dadd], n, layout, False)
            two = _sweep(dev, det, [U, A], [dadd, np.zeros(n)], n, layout, True)
            for o, bs in ((one, (0,)), (two, (0, 1))):
                for b in bs:
                    assert np.array_equal(o["inv"][b], X), (tag, "inv", np.argwhere(o["inv"][b] != X)[:5])
                    assert np.array_equal(o["full"][b], A), (tag, "full")
                    assert np.array_equal(o["piv"][b], [d.min(), d.max()]), (tag, o["piv"][b])
            r = dict(cold=one["inv"])
            for entry in ("warm", "long", "batch", "general"):
                single = entry in ("warm", "long")
                o = _warm(dev, det, entry, [U] if single else [U, A], [dadd] if single else [dadd, np.zeros(n)], [X] if single else [X, X], n, layout)
                for b in range(1 if single else 2):
                    assert np.array_equal(o["inv"][b], X), (tag, entry, "inv", np.argwhere(o["inv"][b] != X)[:5])
                    assert o["acc"][b] == 1.0, (tag, entry, o["acc"])
                    assert o["piv"][b][1] == np.diag(A).max(), (tag, entry, o["piv"][b])
                    want = 1.0 / np.diag(X).max()
                    _bounded(o["piv"][b][:1], np.array([want]), np.array([1e-7 * want]), "warm", "pivots[0], exact case", det, (tag, entry))
                if single:
                    assert np.array_equal(o["full"][0], A), (tag, entry, "full")
                r[entry] = o["inv"]
            res[(det, rep)] = r
    _all_equal(res, n)


@pytest.mark.parametrize("n", [17, 49])
def test_spd_inverse_warm_nan_start(dev, n):
    """A NaN planted in prev_inv: the residual's norm is NaN, NaN compares false, the sweep runs -- accepted == 0 and `inv` and the
    pivots carry the cold sweep's bits for the same matrix, from all four warm entries."""
    A0, d0, X0 = _spd(n, n, rel=1e-3)
    A1, d1, X1 = _spd(n, n + 1000, rel=1e-3)
    bad = X0.copy()
    bad[n // 2, n // 3] = np.nan
    res = {}
    for det in LIBS:
        cold = _sweep(dev, det, [A0, A1], [d0, d1], n, "tight", True)
        for rep in range(2):
            r = {}
            for entry in ("warm", "long", "batch", "general"):
                single = entry in ("warm", "long")
                o = _warm(dev, det, entry, [A0] if single else [A0, A1], [d0] if single else [d0, d1], [bad] if single else [bad, X1], n, "odd")
                tag = (n, det, entry)
                assert o["acc"][0] == 0.0, (tag, o["acc"])
                assert _same_bits(o["inv"][0], cold["inv"][0]) and _same_bits(o["piv"][0], cold["piv"][0]), (tag, "not the cold sweep's bits")
                if not single:
                    assert o["acc"][1] == 1.0, (tag, "the neighbour with a clean start is refined", o["acc"])
                r[entry] = o["inv"]
            res[(det, rep)] = r
    _all_equal(res, n)


def test_spd_inverse_rejects(dev):
    """n = 257, ldp != n on the single warm entries, overlapping strides, batch = 33 for the general entry."""
    n = 8
    A, d, X = _spd(n, 3)
    ops = dict(u=_vec(np.zeros(2 * 300 * 300), dev), p=_vec(np.tile(X.ravel(), 40), dev), w=_vec(np.zeros(4096), dev),
               f=_vec(np.zeros(n * n), dev), i=_vec(np.zeros(40 * n * n), dev), pv=_vec(np.zeros(80), dev), a=_vec(np.zeros(40), dev))
    u, p, w, f, i, pv, a = (ops[k].ptr for k in ("u", "p", "w", "f", "i", "pv", "a"))
    for det in LIBS:
        lib = _lib_of(det)
        s = _stream()
        for rc, want in (
                (lib.pm_spd_inverse_f64(u, 257, None, 257, None, i, 257, pv, s), PM_ERANGE),
                (lib.pm_spd_inverse_f64(u, n - 1, None, n, None, i, n, pv, s), PM_EINVAL),
                (lib.pm_spd_inverse_f64(u, n, None, n, None, i, n - 1, pv, s), PM_EINVAL),
                (lib.pm_spd_inverse_batch_f64(u, 257, 257 * 257, None, 257, None, i, 257, 257 * 257, pv, 2, s), PM_ERANGE),
                (lib.pm_spd_inverse_batch_f64(u, n, n, None, n, None, i, n, n * n, pv, 2, s), PM_EINVAL),
                (lib.pm_spd_inverse_batch_f64(u, n, n * n, None, n, None, i, n + 1, n * n, pv, 2, s), PM_EINVAL),
                (lib.pm_spd_inverse_warm_f64(u, n, None, n, p, n + 1, w, f, i, n, pv, s), PM_EINVAL),
                (lib.pm_spd_inverse_warm_f64(u, n, None, n, p, n, w, f, i, n + 1, pv, s), PM_EINVAL),
                (lib.pm_spd_inverse_warm_long_f64(u, n, None, n, p, n + 1, w, f, i, n, pv, s), PM_EINVAL),
                (lib.pm_spd_inverse_warm_f64(u, 257, None, 257, p, 257, w, f, i, 257, pv, s), PM_ERANGE),
                (lib.pm_spd_inverse_warm_batch_f64(u, n, n * n - 1, None, n, p, n * n, w, i, n * n, pv, 2, s), PM_EINVAL),
                (lib.pm_spd_inverse_warm_batch_f64(u, n, n * n, None, n, p, n * n - 1, w, i, n * n, pv, 2, s), PM_EINVAL),
                (lib.pm_spd_inverse_warm_batch_f64(u, n, n * n, None, n, p, n * n, w, i, n * n - 1, pv, 2, s), PM_EINVAL),
                (lib.pm_inverse_warm_batch_f64(u, n, n * n, None, n, p, n * n, w, i, n * n, pv, a, 33, 0, s), PM_ERANGE),
                (lib.pm_inverse_warm_batch_f64(u, n, n * n, None, n, p, n * n, w, i, n * n, pv, None, 2, 0, s), PM_EINVAL)):
            _rejected(rc, want, det, ops, {})


@pytest.fixture(scope="module", autouse=True)
def _report_worst_errors():
    """After the module's tests: the largest error / bound of every bounded comparison that ran, per entry, quantity and library
    (-s shows it).  Not a check of its own: each comparison asserted its bound where it was made."""
    yield
    for key in sorted(WORST):
        ratio, err, bound = WORST[key]
        print("worst %-10s %-24s %-7s err %.3e  bound %.3e  ratio %.2e" % (key + (err, bound, ratio)))
