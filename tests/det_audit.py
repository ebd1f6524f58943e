"""After-the-fact audit of the deterministic build's accumulators (pm_common.h: PM_Q; include/prosper_hip.h: PM_DET_*).

The mode's promise -- the same bits in every run -- rests on two conditions nothing has to wait for a race to check:
  * a sum of multiples of q that stays below 2^53 q is exact, hence independent of the order of its addends;
  * a finished statistic that is NOT a multiple of its category's quantum proves that an unquantised addend, or one rounded
    with another category's quantum, went in; a category whose sum of |addend| exceeds the bound the host installed proves the
    bound wrong.
This module holds the arithmetic (quantum / pm_q / is_multiple), a recorder that wraps ONE model instance's `_det_set` and
`_call` (and can make the quanta coarse on purpose), the block maps of the packed statistics buffers, and the checks.  A plain
module: no fixtures, no pytest settings."""
import collections
import contextlib
import math

import numpy as np


# ------------------------------------------------------------------------------------------------------ the arithmetic
def quantum(magic):
    """1.5 * 2^e -> 2^(e-52), the spacing of doubles next to the magic constant; 0.0 -> None (PM_Q rounds nothing)."""
    magic = float(magic)
    if magic == 0.0:
        return None
    m, e = math.frexp(magic)            # magic = m * 2^e, m in [0.5, 1): 1.5 * 2^k = 0.75 * 2^(k+1)
    assert m == 0.75, "not a magic constant 1.5 * 2^e: %r" % magic
    return math.ldexp(1.0, e - 1 - 52)


def magic_of(bound):
    """The host's rule (DeviceCAModel._magic): 1.5 * 2^e with 2^(e-1) >= bound."""
    b = float(bound)
    if not np.isfinite(b) or b <= 0.0:
        return 0.0
    return 1.5 * 2.0 ** (int(np.ceil(np.log2(b))) + 1)


def pm_q(v, magic):
    """NumPy twin of PM_Q: (v + M) - M in f64 (round to nearest multiple of the quantum, ties to even)."""
    v = np.asarray(v, dtype=np.float64)
    M = np.float64(magic)
    return (v + M) - M


def is_multiple(x, q):
    """Element-wise: is x a multiple of q?  fmod is exact, and q is a power of two."""
    return np.fmod(np.asarray(x, dtype=np.float64), np.float64(q)) == 0.0


# ---------------------------------------------------------------------------------------------------------- the recorder
class Record(object):
    def __init__(self):
        self.bounds = {}        # unit -> bounds as installed (after the shifts)
        self.magics = {}        # unit -> the eight magic constants
        self.installs = []      # every (unit, bounds) in order
        self.calls = []         # every C entry point enqueued through model._call
        self.args = {}          # entry point -> arguments of its last call

    def q(self, unit, cat):
        return quantum(self.magics[unit][cat])

    def bound(self, unit, cat):
        return self.bounds[unit][cat]

    def ran(self, prefix):
        return [c for c in self.calls if c.startswith(prefix)]


UNITS = ("bsc_fused8", "wp_sparse", "gsc", "gemm", "mca", "dsc", "bsc_rows16", "bsc_fused", "bsc_kernels")


@contextlib.contextmanager
def audit(model, shifts=None):
    """Record what `model` installs and enqueues; `shifts[c]`: bounds[c] *= 2**shifts[c] before they are installed (coarse
    quanta on purpose).  Wraps the INSTANCE only.  The host's record of what the library's symbols hold is dropped before and
    after, so this model installs its own quanta and a later model does too."""
    from prosper_amd.em.camodels import _device
    rec = Record()
    inner_set, inner_call = model._det_set, model._call

    def det_set(unit, bounds):
        b = [float(x) for x in bounds]
        if callable(shifts):
            b = [x * 2.0 ** k for x, k in zip(b, shifts(unit, b))]
        elif shifts is not None:
            b = [x * 2.0 ** shifts[c] for c, x in enumerate(b)]
        rec.installs.append((unit, tuple(b)))
        rec.bounds[unit] = tuple(b)
        rec.magics[unit] = tuple([magic_of(x) for x in b] + [0.0] * (8 - len(b)))
        return inner_set(unit, b)

    def call(label, entry, *args):
        rec.calls.append(entry)
        rec.args[entry] = args
        return inner_call(label, entry, *args)

    for u in UNITS:
        _device._DET_QUANTA_SET.pop(u, None)
    model._det_set, model._call = det_set, call
    try:
        yield rec
    finally:
        del model._det_set, model._call
        for u in UNITS:
            _device._DET_QUANTA_SET.pop(u, None)


def aligned_shifts(descending, base=2, step=2):
    """Shifts from the bounds themselves: within a unit the quanta come out exactly `step` bits apart, ascending or descending
    in the category index, whatever the bounds' own magnitudes (category 1 of the BSC kernels, n emax, is 2^9 .. 2^17 above
    category 0, n: fixed shifts four bits apart never put its quantum BELOW category 0's, so a slot of category 0 rounded
    with index 1 would be a multiple in both of those orders).  The largest bound is shifted by `base` bits at least."""
    def shifts(unit, bounds):
        L = [int(np.ceil(np.log2(b))) if b > 0 and np.isfinite(b) else 0 for b in bounds]
        n = len(bounds)
        return [base + step * ((n - 1 - c) if descending else c) + (max(L) - L[c]) for c in range(n)]
    return shifts


# ------------------------------------------------------------------------------------------------------- the block maps
# name, slice of the raw buffer, (unit, category), signed addends?, addends per datapoint and slot (None: not read off the
# kernel -> 1 + H + S, the number of states a datapoint's row pass visits), final: sum |addend| is taken as |stat| in the
# bounds check ("final value only"), exempt: a one-line reason why the slot is no accumulation.
Block = collections.namedtuple("Block", "name sl unit cat signed addends final exempt")


def _b(name, sl, unit, cat, signed=False, addends=None, final=True, exempt=None):
    return Block(name, sl, unit, cat, signed, addends, final, exempt)


def bsc_blocks(H, D, lib, rec, learn_mu=False):
    """[ Wp (H*D) | Wq (H*H) | qdiag (H) | mus (H) | scalars (4) ] (+ the D data sums when 'mu' is learned).  All four BSC
    kernel files share PM_DET_BSC_FUSED8's categories: 0 Wq, qdiag, mus, count; 1 sum q e; 2 sum lse.  The unit is the one
    whose kernel accumulated the rows (from the recorded calls); Wp: the sparse product, or the dense one (gemm, category 0)
    when it did the work."""
    o_wq, o_qd = lib.pm_bsc_stats_offset_wq(H, D), lib.pm_bsc_stats_offset_qdiag(H, D)
    o_mus, o_sc = lib.pm_bsc_stats_offset_mus(H, D), lib.pm_bsc_stats_offset_scalars(H, D)
    n = lib.pm_bsc_stats_len(H, D)
    if rec.ran("pm_bsc_mstep_rows16"):                  # (the M-step's own pass: an E-step pass before it carried none)
        unit = "bsc_rows16"
    elif rec.ran("pm_bsc_mstep_rows_f64"):
        unit = "bsc_kernels"
    elif rec.ran("pm_bsc_estep_fused8") or rec.ran("pm_bsc_defer_apply"):
        unit = "bsc_fused8"
    else:
        unit = "bsc_fused"
    wp_unit = "wp_sparse" if rec.ran("pm_bsc_wp_sparse") else "gemm"
    out = [
        _b("Wp", slice(0, o_wq), wp_unit, 0, signed=True, addends=1, final=False),
        _b("Wq", slice(o_wq, o_qd), unit, 0),
        _b("qdiag", slice(o_qd, o_mus), unit, 0),
        _b("mus", slice(o_mus, o_sc), unit, 0),
        _b("sum_qe", slice(o_sc, o_sc + 1), unit, 1),
        _b("sum_lse", slice(o_sc + 1, o_sc + 2), unit, 2, signed=True, addends=1, final=False),
        _b("kept", slice(o_sc + 2, o_sc + 3), unit, 0, addends=1),
        _b("overflowed", slice(o_sc + 3, o_sc + 4), unit, 0, addends=1,
           exempt="a counter of overflowed non-zero lists (the gate of the dense product), not a statistic"),
    ]
    if learn_mu:
        out.append(_b("data_sum", slice(n, n + D), "gemm", 1, signed=True, addends=1, final=False))
    return out, dict(o_wq=o_wq, o_qd=o_qd, o_mus=o_mus, o_sc=o_sc, n=n)


def dsc_blocks(H, D, lib, rec, max_k, table_only=False):
    """[ Wp (H*D) | Wq upper triangle, multi-cause part (H*H) | Wq diagonal, singleton part (H) | counts (PM_DSC_MAX_K) |
    sum q e, sum lse, kept, overflowed rows ].  PM_DET_DSC: 0 Wq, diagonal, counts, kept; 1 sum q e; 2 sum lse.  Wp: the sparse
    product (wp_sparse 0) or the dense one (gemm 0).  `table_only`: TSC, whose flag makes the same kernels read every state
    from the table."""
    o_wq, o_qd, o_cnt, o_sc = H * D, H * D + H * H, H * D + H * H + H, H * D + H * H + H + max_k
    assert lib.pm_dsc_stats_len(H, D) == o_sc + 4
    wp_unit = "wp_sparse" if rec.ran("pm_wp_sparse") else "gemm"
    return [
        _b("Wp", slice(0, o_wq), wp_unit, 0, signed=True, addends=1, final=False),
        _b("Wq", slice(o_wq, o_qd), "dsc", 0, signed=True),
        _b("qdiag", slice(o_qd, o_cnt), "dsc", 0,
           exempt="TSC: every state is a row of the table, the whole of Wq (diagonal included) is in the Wq block" if table_only else None),
        _b("counts", slice(o_cnt, o_sc), "dsc", 0),
        _b("sum_qe", slice(o_sc, o_sc + 1), "dsc", 1),
        _b("sum_lse", slice(o_sc + 1, o_sc + 2), "dsc", 2, signed=True, addends=1, final=False),
        _b("kept", slice(o_sc + 2, o_sc + 3), "dsc", 0, addends=1),
        _b("overflowed", slice(o_sc + 3, o_sc + 4), "dsc", 0, addends=1,
           exempt="a counter of overflowed non-zero lists (the gate of the dense product), not a statistic"),
    ], dict(o_wq=o_wq, o_qd=o_qd, o_cnt=o_cnt, o_sc=o_sc)


def gsc_blocks(H, D):
    """GSC's packed buffer as the M-step all-reduces it: [ Wp = Y^T xsz (D*H) | xs^T xsz (H*H) | xsz^T xsz (H*H) | sum xpt_ss
    (H*H) | sum xpt_szsz (H*H) | sum xpt_s (H) | sum xpt_sz (H) | sum |y|^2 ].  The three contractions are the dense product's
    (gemm 0: its K-slices); PM_DET_GSC: 0 xpt_s / xpt_ss, 1 xpt_sz, 2 xpt_szsz (copied from the E-step kernel's buffer by
    pm_gsc_pack_stats_f64, xpt_ss mirrored from its upper triangle)."""
    nWp, nHH = D * H, H * H
    o = nWp + 2 * nHH
    o2 = o + 2 * nHH
    return [
        _b("Wp", slice(0, nWp), "gemm", 0, signed=True, addends=1, final=False),
        _b("xs_xsz", slice(nWp, nWp + nHH), "gemm", 0, signed=True, addends=1, final=False),
        _b("xsz_xsz", slice(nWp + nHH, o), "gemm", 0, signed=True, addends=1, final=False),
        _b("sum_ss", slice(o, o + nHH), "gsc", 0),
        _b("sum_zz", slice(o + nHH, o2), "gsc", 2, signed=True, final=False),
        _b("sum_s", slice(o2, o2 + H), "gsc", 0),
        _b("sum_sz", slice(o2 + H, o2 + 2 * H), "gsc", 1, signed=True, final=False),
        _b("sum_yy", slice(o2 + 2 * H, o2 + 2 * H + 1), "gsc", 0,
           exempt="sum |y_n|^2: a constant of the shard, summed once by the host layer -- no atomics"),
    ], dict(nWp=nWp, nHH=nHH, o=o, o2=o2, n=o2 + 2 * H + 1)


def mca_blocks(H, D, lib, rec):
    """[ G1 = Q1^T Y (H*D) | Wp_multi (H*D) | Wq_multi (H*D) | q1sum (H) | pi, sum q e, sum lse, kept ] (the scratch tail
    behind them is cleared before the kernels return).  PM_DET_MCA: 0 Wq, 1 Wp, 2 pi (q1sum, sum E|s|, kept), 3 sum q e,
    4 sum lse; G1 is the dense product's (gemm 0)."""
    HD = H * D
    o_sc = 3 * HD + H
    assert lib.pm_mca_stats_len(H, D) >= o_sc + 4
    return [
        _b("G1", slice(0, HD), "gemm", 0, signed=True, addends=1, final=False),
        _b("Wp_multi", slice(HD, 2 * HD), "mca", 1, signed=True),
        _b("Wq_multi", slice(2 * HD, 3 * HD), "mca", 0),
        _b("q1sum", slice(3 * HD, o_sc), "mca", 2, addends=1),
        _b("pi", slice(o_sc, o_sc + 1), "mca", 2),
        _b("sum_qe", slice(o_sc + 1, o_sc + 2), "mca", 3),
        _b("sum_lse", slice(o_sc + 2, o_sc + 3), "mca", 4, signed=True, addends=1, final=False),
        _b("kept", slice(o_sc + 3, o_sc + 4), "mca", 2, addends=1),
        _b("scratch", slice(o_sc + 4, int(lib.pm_mca_stats_len(H, D))), "mca", 0,
           exempt="the per-XCD scratch copies: folded into Wp_multi | Wq_multi and cleared before the kernels return"),
    ], dict(HD=HD, o_sc=o_sc)


# ------------------------------------------------------------------------------------------------------------ the checks
def check_block(name, x, q, min_quanta=64.0):
    """Every entry a multiple of q, and the pass is not vacuous: the block is not all zero and at least half of its non-zero
    entries are >= `min_quanta` quanta in magnitude (else being a multiple proves little).  Returns a list of complaints."""
    x = np.asarray(x, dtype=np.float64).ravel()
    bad = []
    if q is None:
        return ["%s: no quantum installed for its category" % name]
    if not np.isfinite(x).all():
        return ["%s: non-finite entries" % name]
    mult = is_multiple(x, q)
    if not mult.all():
        i = int(np.flatnonzero(~mult)[0])
        bad.append("%s: %d of %d entries are no multiple of the quantum 2^%d (first: [%d] = %r, remainder %.3e quanta)"
                   % (name, int((~mult).sum()), x.size, int(np.log2(q)), i, x[i], math.fmod(x[i], q) / q))
    nz = x[x != 0.0]
    if nz.size == 0:
        bad.append("%s: all zero -- nothing was accumulated, the check is vacuous" % name)
    elif (np.abs(nz) >= min_quanta * q).sum() * 2 < nz.size:
        bad.append("%s: only %d of %d non-zero entries reach %g quanta (2^%d): the check is vacuous"
                   % (name, int((np.abs(nz) >= min_quanta * q).sum()), nz.size, min_quanta, int(np.log2(q))))
    return bad


def check_multiples(raw, blocks, rec):
    """check_block over a block map, each block against the quantum recorded for its (unit, category)."""
    raw = np.asarray(raw, dtype=np.float64)
    bad = []
    for b in blocks:
        if b.exempt:
            continue
        bad += check_block(b.name, raw[b.sl], rec.q(b.unit, b.cat))
    return bad


def close_tol(block, rec, N, K, ref):
    """|got - ref| <= A N q / 2 + 1e-9 max|ref|: half a quantum per addend (A addends per datapoint and slot; 1 + H + S = K
    where the kernel does not say), plus the suite's rounding term for the plain sums."""
    A = block.addends if block.addends is not None else K
    return A * N * rec.q(block.unit, block.cat) / 2.0 + 1e-9 * float(np.abs(np.asarray(ref, dtype=np.float64)).max())


def fsum_cols(X):
    """Column sums of a 2-D array in extended precision (np.longdouble), returned as longdouble."""
    return np.asarray(X, dtype=np.longdouble).sum(axis=0)
