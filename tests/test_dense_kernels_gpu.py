"""The dense kernels (gemm_f64.hip, gemm_small.hip) through the C ABI, on strided, padded and 8-byte-aligned operands, at one
shape per dispatch path -- asserted with pm_gemm_nt_plan / pm_gemm_tn_plan --, compared EXACTLY.

Harness.  Every operand is placed by ``embed`` inside a larger device buffer filled with one recognisable NaN: at least 128
guard rows of ``ld`` doubles in front and behind, the padding columns [width, ld) of every row, and (for outputs that are
not accumulated into) the result block itself.  After a call the result block is compared, every other double of the output
buffer must still be the sentinel bit for bit, and the operand buffers must be unchanged.  A store past N or M, a row that is
over-read and masked by multiplication, a clamped row that reaches the result: each one shows.

Exact arithmetic.  Inputs are integers in [-8, 8] that depend on their position ((i + 3 j) % 5 added to a seeded draw: not
symmetric, so a transposed or swapped tile map changes the answer).  Every product and every partial sum up to K = 8192 is an
integer far below 2^53, so every summation order -- MFMA chains, K-slices met in f64 atomics, the fused launch, the gathered
kernel, the column reductions -- gives the same bits as NumPy's f64 product, and the comparison is equality.

Plan bit -> the case that asserts it (``nt_path_cases`` / ``tn_path_cases`` of test_gemm_plan_cpu.py; shapes at 512 slots):
  PM_NT_PLAN_DMA_MAIN        main (16384, 512, 8), rest64; both builds
  PM_NT_PLAN_DMA_REST        rest (64, 100, 48), both builds; split (200, 256, 1024) in the deterministic build
  PM_NT_PLAN_DMA_REST_SPLIT  split (200, 256, 1024); default build only (the deterministic build never splits K)
  PM_NT_PLAN_DMA_FUSED       fused (16517, 512, 128); default build only
  PM_NT_PLAN_DMA_REST64      rest64 (10245, 1024, 8); default build only
  PM_NT_PLAN_DMA_WHOLE       fused and rest64 in the deterministic build (its one-launch form); that build only
  PM_NT_PLAN_REG_MT1         mt1_al (130, 129, 18), mt1_un (333, 10, 25), mt1_odd_base (200, 256, 1024 at an 8-byte base)
  PM_NT_PLAN_REG_MT2         mt2_un (4128, 500, 9), mt2_al (.., 18)
  PM_NT_PLAN_REG_MT4         mt4_un (8200, 512, 9), mt4_al (.., 18), mt4_one (1, 1, 1), mt4_odd_base (32, 16, 8 at an 8-byte base)
  PM_NT_PLAN_ALIGNED         every DMA case, mt1_al, mt2_al, mt4_al; its absence in the *_un and *_odd_base cases
  PM_TN_PLAN_DMA             dma (128, 128, 64), dma_tail, dma_remap
  PM_TN_PLAN_TAIL            dma_tail (128, 128, 71)
  PM_TN_PLAN_REMAP           dma_remap (128, 256, 1024), reg_remap (130, 128, 1024)
  PM_TN_PLAN_REG             reg_al_edge_m (130, 128, 64), reg_al_short_k (128, 128, 63), reg_un (33, 7, 5), reg_odd_base
  PM_TN_PLAN_ALIGNED         the dma cases and reg_al_*; its absence in reg_un and reg_odd_base
(test_nt_paths and test_tn_paths run every case on both libraries.)

Rounding.  ``test_rounding_bound`` runs standard-normal operands through one shape per kernel family and holds every element
to the textbook componentwise bound against an 80-bit reference: |C - Chat| <= (K + 2) 2^-53 (|A| |B|^T), for the accumulating
forms (K + 3) 2^-53 (|A|^T |B| + |C0|)."""
import ctypes
import functools

import numpy as np
import pytest

from test_gemm_plan_cpu import (NT_ALIGNED, NT_FUSED, NT_MAIN, NT_MT1, NT_MT2, NT_MT4, NT_REST, NT_REST64, NT_REST_SPLIT,
                                NT_WHOLE, PM_ERANGE, TN_ALIGNED, TN_DMA, TN_REG, nt_path_cases, nt_plan, tn_path_cases,
                                tn_plan)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = 0x7FF8DEADBEEF0001          # a quiet NaN with a payload no arithmetic produces
GUARD_ROWS = 128
NT_DMA_BITS = NT_MAIN | NT_REST | NT_REST_SPLIT | NT_FUSED | NT_REST64 | NT_WHOLE
U = 2.0 ** -53

if np.finfo(np.longdouble).nmant >= 63:
    def _matmul_hi(A, B):
        """A . B in 80-bit arithmetic, rounded to f64 per element only by the caller's subtraction."""
        return A.astype(np.longdouble) @ B.astype(np.longdouble)
else:                                                     # pragma: no cover  (platforms whose long double is a double)
    import mpmath

    def _matmul_hi(A, B):
        mpmath.mp.prec = 113
        Bt = [[mpmath.mpf(float(v)) for v in B[:, j]] for j in range(B.shape[1])]
        return np.array([[float(mpmath.fdot([mpmath.mpf(float(v)) for v in A[i]], Bt[j])) for j in range(B.shape[1])]
                         for i in range(A.shape[0])])


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU box (MI355X)")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def slots(dev):
    s = 2 * torch.cuda.get_device_properties(dev).multi_processor_count
    assert nt_plan(1, 1, 1, 0)[1][0] == s and nt_plan(1, 1, 1, 0, det=True)[1][0] == s
    return s


@pytest.fixture(scope="module")
def det_quanta(dev):
    """The deterministic library rounds the addends of its atomics to the quanta its caller installed (pm_det_set_quanta;
    unit `gemm`: the K-slices of the accumulating products and the column reductions).  Bound 2^40: a quantum of 2^-11, of
    which every integer is a multiple -- the rounding is then the identity on this module's data.  The host layer's
    record of what is installed is dropped before and after, so that a model of a later test installs its own."""
    from prosper_amd import _lib
    from prosper_amd.em.camodels import _device
    M8 = (ctypes.c_double * 8)(*([1.5 * 2.0 ** 41] * 8))
    _device._DET_QUANTA_SET.pop("gemm", None)
    _lib.call("pm_det_set_quanta", _lib.DET_UNITS["gemm"], M8, _stream(), det=True)
    torch.cuda.synchronize()
    yield M8
    _device._DET_QUANTA_SET.pop("gemm", None)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ints(rows, cols, seed):
    """Position-dependent integers in [-8, 8] as f64."""
    rng = np.random.RandomState(seed)
    i, j = np.arange(rows)[:, None], np.arange(cols)[None, :]
    return (rng.randint(-8, 5, size=(rows, cols)) + (i + 3 * j) % 5).astype(np.float64)


def _t(x):
    """A host array as a (writable, contiguous) CPU tensor of its own."""
    return torch.from_numpy(np.array(x, dtype=np.float64, order="C"))


class Embedded:
    """A host matrix inside a sentinel-filled device buffer (see ``embed``)."""

    def __init__(self, array, ld, offset_doubles, dev, fill_block=True):
        rows, cols = array.shape
        assert ld >= cols and offset_doubles in (0, 1)
        self.rows, self.cols, self.ld = rows, cols, ld
        self.start = GUARD_ROWS * ld + offset_doubles
        self.buf = torch.empty(self.start + (rows + GUARD_ROWS) * ld + 2, dtype=torch.float64, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.buf.view(torch.int64).fill_(SENTINEL)
        if fill_block:
            self.block().copy_(_t(array))
        self.before = self.buf.clone()

    def block(self):
        return self.buf[self.start:self.start + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols]

    @property
    def addr(self):
        return self.buf.data_ptr() + 8 * self.start

    @property
    def ptr(self):
        return ctypes.c_void_p(self.addr)

    @property
    def aligned(self):
        """What the launchers ask of an operand before they use 16-byte loads on it."""
        return self.addr % 16 == 0 and self.ld % 2 == 0

    def unchanged(self):
        return torch.equal(self.buf.view(torch.int64), self.before.view(torch.int64))

    def outside_untouched(self):
        """Every guard row and padding column still holds the sentinel, bit for bit."""
        rest = self.buf.view(torch.int64).clone()
        rest[self.start:self.start + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols] = SENTINEL
        return bool((rest == SENTINEL).all())


def embed(array, ld, offset_doubles, dev, fill_block=True):
    """``array`` at ``offset_doubles`` (0: a 16-byte-aligned base, 1: an 8-byte-aligned one) behind 128 guard rows of ``ld``
    doubles, followed by as many, row stride ``ld``; every double that is not an element of the matrix is the sentinel NaN.
    ``fill_block=False``: the matrix is sentinel too (an output a kernel must write completely)."""
    return Embedded(array, ld, offset_doubles, dev, fill_block)


def _ld(width, pad):
    """pad: doubles added to the row; "ev": the smallest even stride with at least one padding column."""
    if pad == "ev":
        return width + 2 if width % 2 == 0 else width + 1
    return width + pad


# name -> ((pad, offset) of A, of B, of C)
LAYOUTS = {
    "tight": ((0, 0), (0, 0), (0, 0)),
    "even2": ((2, 0), (2, 0), (2, 0)),
    "even6": ((6, 0), (6, 0), (6, 0)),
    "padA": ((6, 0), (0, 0), (0, 0)),
    "padB": ((0, 0), (2, 0), (0, 0)),
    "padC": ((0, 0), (0, 0), (6, 0)),
    "odd": ((1, 0), (1, 0), (1, 0)),
    "oddC": ((0, 0), (0, 0), (1, 0)),
    "off1": (("ev", 1), ("ev", 1), ("ev", 1)),
    "off1A": (("ev", 1), (2, 0), (2, 0)),
    "off1B": ((2, 0), ("ev", 1), (0, 0)),
    "off1C": ((0, 0), (0, 0), ("ev", 1)),
}
FEW_LAYOUTS = ["tight", "even6", "padC", "odd", "off1"]        # for the shapes with tens of megabytes of C


def _describe(got, ref):
    bad = (got != ref) | torch.isnan(got)
    n = int(bad.sum())
    idx = torch.nonzero(bad)[:5].tolist()
    return "%d of %d elements differ, first at %s: got %s, want %s" % (
        n, bad.numel(), idx, [float(got[i, j]) for i, j in idx], [float(ref[i, j]) for i, j in idx])


@functools.lru_cache(maxsize=None)
def _operands(kind, M, N, K):
    """Integer operands and the exact product, once per shape.  kind: "nt" C = A B^T (A: M x K, B: N x K), "nn" C = A B
    (B: K x N), "tn" C = C0 + A^T B (A: K x M, B: K x N)."""
    seed = (M * 31 + N * 7 + K) % (2 ** 31)
    if kind == "nt":
        A, B = ints(M, K, seed), ints(N, K, seed + 1)
        ref, C0 = A @ B.T, None
    elif kind == "nn":
        A, B = ints(M, K, seed), ints(K, N, seed + 1)
        ref, C0 = A @ B, None
    else:
        A, B, C0 = ints(max(K, 1), M, seed)[:K], ints(max(K, 1), N, seed + 1)[:K], ints(M, N, seed + 2) * 3.0
        ref = C0 + A.T @ B
    for x in (A, B, ref):
        x.setflags(write=False)
    return A, B, C0, ref


def run_gemm(dev, kind, entry, M, N, K, layout, det=False, gate=None, want_mask=None, expect_skip=False):
    """Embed the operands of one call in ``layout``, run ``entry``, and check the result block (exact), the sentinel around
    C and the operands.  Returns (plan mask or None, all three operands aligned)."""
    from prosper_amd import _lib
    A, B, C0, ref = _operands(kind, M, N, K)
    (pa, oa), (pb, ob), (pc, oc) = LAYOUTS[layout] if isinstance(layout, str) else layout
    what = "%s %s (%d, %d, %d) layout %s det=%s" % (entry, kind, M, N, K, layout, det)
    ea = embed(A, _ld(A.shape[1], pa), oa, dev)
    eb = embed(B, _ld(B.shape[1], pb), ob, dev)
    ec = embed(ref if C0 is None else C0, _ld(N, pc), oc, dev, fill_block=C0 is not None)
    aligned = ea.aligned and eb.aligned
    mask = None
    if entry == "pm_gemm_nt_f64":
        mask = nt_plan(M, N, K, aligned, det)[0]
    elif entry.startswith("pm_gemm_tn_acc"):
        mask = tn_plan(M, N, K, aligned, det)[0]
    if want_mask is not None:
        assert mask == want_mask, "%s: plan %#x, expected %#x" % (what, mask, want_mask)
    args = [ea.ptr, ea.ld, eb.ptr, eb.ld, ec.ptr, ec.ld, M, N, K]
    if entry == "pm_gemm_tn_acc_gated_f64":
        args.append(ctypes.c_void_p(gate.data_ptr()))
    _lib.call(entry, *args, _stream(), det=det)
    torch.cuda.synchronize()
    want = _t(C0 if expect_skip else ref).to(dev)
    got = ec.block()
    assert torch.equal(got, want), what + ": " + _describe(got, want)
    assert ec.outside_untouched(), what + ": a guard row or padding column of C was written"
    assert ea.unchanged() and eb.unchanged(), what + ": an operand was modified"
    return mask, aligned


# ------------------------------------------------------------------------------------------------ pm_gemm_nt_f64
@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
@pytest.mark.parametrize("name", sorted(nt_path_cases(512)))
def test_nt_paths(dev, slots, name, det):
    """One shape per path of pm_gemm_nt_f64, the path asserted with pm_gemm_nt_plan, in both libraries; then the same shape
    in other layouts (whichever kernel those route to: an odd stride or an 8-byte base may not reach an LDS-DMA kernel or
    an aligned flavour, and the plan must say so)."""
    M, N, K, aligned, want, want_det = nt_path_cases(slots)[name]
    first = "tight" if aligned else "off1"
    run_gemm(dev, "nt", "pm_gemm_nt_f64", M, N, K, first, det, want_mask=want_det if det else want)
    big = M * N > 2 ** 20
    for layout in (FEW_LAYOUTS if big else LAYOUTS):
        if layout == first:
            continue
        mask, al = run_gemm(dev, "nt", "pm_gemm_nt_f64", M, N, K, layout, det)
        if not al or K % 2:
            assert mask & (NT_DMA_BITS | NT_ALIGNED) == 0, (name, layout, hex(mask))
        elif K % 8 == 0:
            assert mask & NT_DMA_BITS and mask & NT_ALIGNED, (name, layout, hex(mask))
        else:
            assert mask & NT_ALIGNED and mask & (NT_MT1 | NT_MT2 | NT_MT4), (name, layout, hex(mask))


def test_nt_unaligned_base_with_k_mod_8_routes_to_register_kernels(dev, slots):
    """An 8-byte-aligned A or B with even strides and K % 8 == 0 -- everything the LDS-DMA kernels need except the base --
    runs the register-staged kernel in its scalar-load flavour, in both libraries; an 8-byte-aligned C changes nothing."""
    for det in (False, True):
        for layout in ("off1", "off1A", "off1B"):
            mask, al = run_gemm(dev, "nt", "pm_gemm_nt_f64", 200, 256, 1024, layout, det)
            assert not al and mask == NT_MT1, (layout, hex(mask))
        mask, al = run_gemm(dev, "nt", "pm_gemm_nt_f64", 200, 256, 1024, "off1C", det)
        assert al and mask & NT_DMA_BITS, hex(mask)


# rows ending 1, 63, 64 and 65 into a 128-row tile (and into a 64-row half); column tiles with 1, 8 and 9 of their 16-column
# blocks inside N, and ragged ones
EDGE_MN = [(129, 16), (191, 128), (192, 144), (193, 129), (63, 10), (1, 144), (64, 136), (65, 72)]
# K: 8 .. 40 are 1, 2, 3 and 5 K-steps of the 4-stage LDS-DMA ring; 9, 18, 33, 50 the register-staged kernels (odd / even K,
# 1 .. 4 K-steps of 16 with a ragged last one)
EDGE_SHAPES = ([(m, n, k) for m, n in EDGE_MN for k in (16, 9, 18)] +
               [(129, 16, 8), (193, 129, 24), (65, 72, 40), (63, 10, 33), (192, 144, 50)])


@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
@pytest.mark.parametrize("M,N,K", EDGE_SHAPES)
def test_nt_edges_in_every_layout(dev, M, N, K, det):
    for layout in LAYOUTS:
        run_gemm(dev, "nt", "pm_gemm_nt_f64", M, N, K, layout, det)


@pytest.mark.parametrize("M,N,K", EDGE_SHAPES)
def test_nt_rows_edges_in_every_layout(dev, M, N, K):
    """pm_gemm_nt_rows_f64: one launch, whole K per tile (LDS-DMA kernel or the 128-row register-staged one)."""
    for layout in LAYOUTS:
        run_gemm(dev, "nt", "pm_gemm_nt_rows_f64", M, N, K, layout)
    run_gemm(dev, "nt", "pm_gemm_nt_rows_f64", M, N, K, "tight", det=True)
    run_gemm(dev, "nt", "pm_gemm_nt_rows_f64", M, N, K, "off1", det=True)


@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
@pytest.mark.parametrize("M,N,K,off", [(300, 144, 64, 0), (300, 144, 50, 0), (300, 144, 64, 1), (700, 72, 9, 0)])
def test_nt_rows_row_contract(dev, M, N, K, off, det):
    """a row of C is a function of its row of A and of B alone.  Permute the rows of A (non-integer data) and
    the rows of C permute bit for bit; a single row computed alone has the same bits too."""
    from prosper_amd import _lib
    rng = np.random.RandomState(M + N + K)
    A, B = rng.normal(size=(M, K)), rng.normal(size=(N, K))
    perm = rng.permutation(M)
    eb = embed(B, _ld(K, "ev"), off, dev)
    outs = []
    for rows in (A, A[perm], A[5:6]):
        ea = embed(rows, _ld(K, "ev"), off, dev)
        ec = embed(np.zeros((rows.shape[0], N)), N + 1, 0, dev, fill_block=False)
        _lib.call("pm_gemm_nt_rows_f64", ea.ptr, ea.ld, eb.ptr, eb.ld, ec.ptr, ec.ld, rows.shape[0], N, K, _stream(),
                  det=det)
        torch.cuda.synchronize()
        assert ec.outside_untouched() and ea.unchanged() and eb.unchanged()
        outs.append(ec.block().cpu().numpy())
    assert not np.isnan(outs[0]).any()
    assert np.array_equal(outs[1], outs[0][perm])
    assert np.array_equal(outs[2][0], outs[0][5])


# ------------------------------------------------------------------------------------------------ pm_gemm_nt_small_f64
# per_wave = ceil(ceil(K / 16) / 8) chunks per wavefront picks the unroll: K = 16 -> 1, 256 -> 2, 512 -> 4, 1040 -> 9 (> 4);
# K % 4 != 0 (18, 25, 1030) and a misaligned layout take the scalar-load flavour (unroll 2 or 8); K % 16 in {4, 12}
# (20, 28, 268, 516) end in a chunk of which only the first one or three lane groups hold columns
NT_SMALL_SHAPES = [(100, 37, 16), (17, 130, 256), (33, 50, 512), (20, 19, 1040), (100, 37, 18), (17, 33, 25), (5, 40, 1030),
                   (30, 30, 20), (31, 47, 28), (16, 16, 268), (1, 1, 516), (1, 1, 1), (48, 32, 4)]


@pytest.mark.parametrize("M,N,K", NT_SMALL_SHAPES)
def test_nt_small_in_every_layout(dev, M, N, K):
    for layout in LAYOUTS:
        run_gemm(dev, "nt", "pm_gemm_nt_small_f64", M, N, K, layout)
    run_gemm(dev, "nt", "pm_gemm_nt_small_f64", M, N, K, "even2", det=True)


def test_nt_small_limits(dev):
    """M, N <= 1024: the largest grid, and PM_ERANGE past it with C untouched."""
    from prosper_amd import _lib
    run_gemm(dev, "nt", "pm_gemm_nt_small_f64", 1024, 1000, 8, "even2")
    a, c = embed(ints(1025, 4, 0), 4, 0, dev), embed(np.zeros((1025, 4)), 4, 0, dev, fill_block=False)
    for M, N in ((1025, 4), (4, 1025)):
        assert _lib.load().pm_gemm_nt_small_f64(a.ptr, 4, a.ptr, 4, c.ptr, max(N, 4), M, N, 4, _stream()) == PM_ERANGE
    torch.cuda.synchronize()
    assert c.unchanged()


@pytest.mark.parametrize("M,K,pad,off", [(50, 64, 0, 0), (130, 268, 2, 0), (16, 8, 6, 0), (37, 25, 1, 0), (130, 64, "ev", 1),
                                          (1024, 4, 0, 0)])
def test_nt_small_gram_shortcut(dev, M, K, pad, off):
    """A == B, lda == ldb, M == N: only tiles on or above the diagonal compute and store their mirror image.  With ldc > N
    the mirror stores must stay inside [M, N); the result is exact here and bit-symmetric on non-integer data.  The same
    pointer with M != N is NOT the shortcut: rows [0, N) of the one operand serve as B."""
    from prosper_amd import _lib
    A = ints(M, K, M + K)
    ea = embed(A, _ld(K, pad), off, dev)
    for ldc in (M, M + 1, M + 6):
        ec = embed(np.zeros((M, M)), ldc, 0, dev, fill_block=False)
        _lib.call("pm_gemm_nt_small_f64", ea.ptr, ea.ld, ea.ptr, ea.ld, ec.ptr, ldc, M, M, K, _stream())
        torch.cuda.synchronize()
        want = torch.from_numpy(A @ A.T).to(dev)
        assert torch.equal(ec.block(), want), _describe(ec.block(), want)
        assert ec.outside_untouched() and ea.unchanged()
    N = max(1, M - 16 - 3)
    ec = embed(np.zeros((M, N)), N + 3, 1, dev, fill_block=False)
    _lib.call("pm_gemm_nt_small_f64", ea.ptr, ea.ld, ea.ptr, ea.ld, ec.ptr, ec.ld, M, N, K, _stream())
    torch.cuda.synchronize()
    want = torch.from_numpy(A @ A[:N].T).to(dev)
    assert torch.equal(ec.block(), want), _describe(ec.block(), want)
    assert ec.outside_untouched() and ea.unchanged()
    # bit symmetry where rounding exists
    R = np.random.RandomState(M).normal(size=(M, K))
    er = embed(R, _ld(K, pad), off, dev)
    ec = embed(np.zeros((M, M)), M + 2, 0, dev, fill_block=False)
    _lib.call("pm_gemm_nt_small_f64", er.ptr, er.ld, er.ptr, er.ld, ec.ptr, ec.ld, M, M, K, _stream())
    torch.cuda.synchronize()
    G = ec.block().cpu().numpy()
    assert not np.isnan(G).any() and np.array_equal(G, G.T)
    assert ec.outside_untouched() and er.unchanged()


# ------------------------------------------------------------------------------------------------ pm_gemm_nn_small_f64
# the four unrolls (K = 16, 256, 512, 1040), K % 4 != 0, N = 1, 15, 16, 17, and one product across the 65536-column slab;
# `al` (16-byte loads of A) goes off with an odd lda or an 8-byte base: the layouts; ldb > N: padB, even2, ...
NN_SMALL_SHAPES = [(7, 1, 16), (20, 15, 256), (33, 16, 512), (5, 17, 1040), (16, 17, 18), (3, 65536 + 17, 5), (40, 33, 12),
                   (1, 1, 1)]


@pytest.mark.parametrize("M,N,K", NN_SMALL_SHAPES)
def test_nn_small_in_every_layout(dev, M, N, K):
    for layout in LAYOUTS:
        run_gemm(dev, "nn", "pm_gemm_nn_small_f64", M, N, K, layout)
    run_gemm(dev, "nn", "pm_gemm_nn_small_f64", M, N, K, "even2", det=True)


def test_nn_small_limits(dev):
    from prosper_amd import _lib
    run_gemm(dev, "nn", "pm_gemm_nn_small_f64", 1024, 20, 8, "padB")
    a, c = embed(ints(1025, 4, 0), 4, 0, dev), embed(np.zeros((1025, 4)), 4, 0, dev, fill_block=False)
    assert _lib.load().pm_gemm_nn_small_f64(a.ptr, 4, a.ptr, 4, c.ptr, 4, 1025, 4, 4, _stream()) == PM_ERANGE
    torch.cuda.synchronize()
    assert c.unchanged()


# ------------------------------------------------------------------------------------------------ pm_gemm_tn_acc(_gated)_f64
TN_MORE = [(10, 25, 333), (256, 128, 200), (128, 128, 2055), (100, 48, 1000), (2, 2, 17), (129, 130, 40)]


@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
@pytest.mark.parametrize("name", sorted(tn_path_cases()))
def test_tn_paths(dev, slots, det_quanta, name, det):
    """One shape per path of pm_gemm_tn_acc_f64 (asserted with pm_gemm_tn_plan), C starting from integers, in both
    libraries; then the other layouts."""
    M, N, K, aligned, want, _ = tn_path_cases()[name]
    first = "tight" if aligned else "off1"
    run_gemm(dev, "tn", "pm_gemm_tn_acc_f64", M, N, K, first, det, want_mask=want)
    for layout in LAYOUTS:
        if layout == first:
            continue
        mask, al = run_gemm(dev, "tn", "pm_gemm_tn_acc_f64", M, N, K, layout, det)
        if not al:
            assert mask & (TN_DMA | TN_ALIGNED) == 0 and mask & TN_REG, (name, layout, hex(mask))
        elif aligned:               # (remap and tail bits aside: the same kernel family)
            assert mask & ~0x18 == want & ~0x18, (name, layout, hex(mask))


@pytest.mark.parametrize("M,N,K", TN_MORE)
def test_tn_more_shapes_in_every_layout(dev, det_quanta, M, N, K):
    """Several K-splits with a ragged last one, LDS-DMA with two splits, with 16 splits (remap) plus a tail launch, tiny and
    odd sizes."""
    for layout in LAYOUTS:
        run_gemm(dev, "tn", "pm_gemm_tn_acc_f64", M, N, K, layout)
    run_gemm(dev, "tn", "pm_gemm_tn_acc_f64", M, N, K, "tight", det=True)


def test_tn_k_zero_leaves_c_untouched(dev, det_quanta):
    for det in (False, True):
        run_gemm(dev, "tn", "pm_gemm_tn_acc_f64", 128, 128, 0, "padC", det, want_mask=0, expect_skip=True)
        run_gemm(dev, "tn", "pm_gemm_tn_acc_f64", 33, 7, 0, "odd", det, want_mask=0, expect_skip=True)


@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
@pytest.mark.parametrize("M,N,K,layout", [(128, 128, 71, "tight"), (128, 256, 1024, "padC"), (33, 7, 5, "odd"),
                                           (130, 128, 64, "even2"), (128, 128, 64, "off1")])
def test_tn_gate(dev, det_quanta, M, N, K, layout, det):
    """pm_gemm_tn_acc_gated_f64: the kernels test `*gate == 0.0` on the device.  Both signs of zero compare equal to 0.0,
    so 0.0 and -0.0 leave C bit-identical (every launch of the call: LDS-DMA, its tail, register-staged); 1.0 and any other
    non-zero value run the product."""
    for value, skipped in ((0.0, True), (-0.0, True), (1.0, False), (-2.5, False)):
        gate = torch.tensor([value], dtype=torch.float64, device=dev)
        run_gemm(dev, "tn", "pm_gemm_tn_acc_gated_f64", M, N, K, layout, det, gate=gate, expect_skip=skipped)
        assert float(gate[0]) == value and bool(torch.signbit(gate[0])) == bool(np.signbit(value))


# ------------------------------------------------------------------------------------------------ pm_gemm_tn_acc_rows_f64
def _run_tn_rows(dev, det, M, N, R, max_rows, count, rows, layout, expect=0):
    from prosper_amd import _lib
    (pa, oa), (pb, ob), (pc, oc) = LAYOUTS[layout]
    zero_row = R // 2
    A, B, C0 = ints(R, M, 11), ints(R, N, 12), ints(M, N, 13) * 3.0
    A[zero_row] = 0.0
    B[zero_row] = 0.0
    ea, eb, ec = embed(A, _ld(M, pa), oa, dev), embed(B, _ld(N, pb), ob, dev), embed(C0, _ld(N, pc), oc, dev)
    rows_d = torch.from_numpy(rows.astype(np.int32)).to(dev)
    count_d = torch.tensor([count], dtype=torch.int32, device=dev)
    rc = _lib.load(det).pm_gemm_tn_acc_rows_f64(ea.ptr, ea.ld, eb.ptr, eb.ld, ec.ptr, ec.ld, M, N,
                                                 ctypes.c_void_p(rows_d.data_ptr()), ctypes.c_void_p(count_d.data_ptr()),
                                                 max_rows, zero_row, _stream())
    torch.cuda.synchronize()
    what = "rows (%d, %d) max_rows %d count %d layout %s det=%s" % (M, N, max_rows, count, layout, det)
    assert rc == expect, what
    used = rows[:min(count, max_rows)]
    ref = C0 if expect else C0 + A[used].T @ B[used]            # the plain gather-and-multiply
    want = torch.from_numpy(ref).to(dev)
    assert torch.equal(ec.block(), want), what + ": " + _describe(ec.block(), want)
    assert ec.outside_untouched() and ea.unchanged() and eb.unchanged(), what
    assert int(count_d[0]) == count and np.array_equal(rows_d.cpu().numpy(), rows)


@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
@pytest.mark.parametrize("max_rows", [512, 200])
def test_tn_rows_counts_and_lists(dev, slots, det_quanta, max_rows, det):
    """C += A[rows]^T B[rows] over a device-side list: *count in {0, 1, 7, 8, 9, max_rows, max_rows + 5 (clipped)}, lists in
    descending order with duplicates and with the zero row listed, entries past *count pointing at rows that must not be
    read into the sum.  (128, 256): 2 tiles; max_rows = 512 gives min(slots / 2, 8) = 8 K-splits -- a multiple of 8, the
    XCD remap --, max_rows = 200 gives 4."""
    M, N, R = 128, 256, 300
    assert min(slots // 2, (max_rows + 63) // 64) % 8 == (0 if max_rows == 512 else 4)
    rng = np.random.RandomState(max_rows)
    for count in (0, 1, 7, 8, 9, max_rows, max_rows + 5):
        rows = np.sort(rng.randint(0, R, size=max_rows))[::-1].copy()
        rows[1::7] = rows[0::7][:len(rows[1::7])]                       # duplicates
        if count > 2:
            rows[2] = R // 2                                            # the zero row may be listed too
        for layout in ("tight", "even2", "padA", "padB", "padC", "oddC", "off1C"):
            _run_tn_rows(dev, det, M, N, R, max_rows, count, rows, layout)


def test_tn_rows_refuses_misaligned_layouts(dev, det_quanta):
    """PM_ERANGE for operands the LDS-DMA kernel cannot load (odd stride, 8-byte base) and for M or N that are not whole
    tiles; C is untouched."""
    rows = np.arange(64)
    for layout in ("odd", "off1", "off1A", "off1B"):
        _run_tn_rows(dev, False, 128, 128, 100, 64, 64, rows, layout, expect=PM_ERANGE)
    _run_tn_rows(dev, False, 130, 128, 100, 64, 64, rows, "even2", expect=PM_ERANGE)
    _run_tn_rows(dev, False, 128, 64, 100, 64, 64, rows, "even2", expect=PM_ERANGE)


# ------------------------------------------------------------------------------------------------ row and column reductions
RED_D = [1, 63, 64, 65, 257]
RED_N = [1, 2, 3, 4097]            # odd N: the tail of the two-row unroll; 4097 rows: more than one pass of the row kernels' grid
RED_LD = [(0, 0), (2, 0), (1, 0), ("ev", 1)]


def _vec(values, dev, fill_block=True):
    """A vector as a 1 x n embedded matrix."""
    return embed(np.asarray(values, dtype=np.float64).reshape(1, -1), len(values), 0, dev, fill_block)


@pytest.mark.parametrize("N", RED_N)
@pytest.mark.parametrize("D", RED_D)
def test_row_norms(dev, D, N):
    """pm_row_sqnorm_f64 and pm_row_wsqnorm_f64 (integer weights): exact, `out` written in [0, N) only."""
    from prosper_amd import _lib
    Y, w = ints(N, D, N + D), np.arange(D) % 4 + 1.0
    for pad, off in RED_LD:
        for det in (False, True):
            ey, ew = embed(Y, _ld(D, pad), off, dev), _vec(w, dev)
            o1, o2 = _vec(np.zeros(N), dev, False), _vec(np.zeros(N), dev, False)
            _lib.call("pm_row_sqnorm_f64", ey.ptr, ey.ld, N, D, o1.ptr, _stream(), det=det)
            _lib.call("pm_row_wsqnorm_f64", ey.ptr, ey.ld, N, D, ew.ptr, o2.ptr, _stream(), det=det)
            torch.cuda.synchronize()
            assert np.array_equal(o1.block().cpu().numpy()[0], (Y * Y).sum(1)), (pad, off, det)
            assert np.array_equal(o2.block().cpu().numpy()[0], (Y * w * Y).sum(1)), (pad, off, det)
            assert o1.outside_untouched() and o2.outside_untouched() and ey.unchanged() and ew.unchanged()


@pytest.mark.parametrize("N", RED_N)
@pytest.mark.parametrize("D", RED_D)
def test_col_moments(dev, det_quanta, D, N):
    """pm_col_moments_f64 in both modes (column sums; squared deviations from an integer centre), accumulated into non-zero
    integer `sums`."""
    from prosper_amd import _lib
    Y, centre, s0 = ints(N, D, N + 2 * D), np.arange(D) % 7 - 3.0, np.arange(D) * 2.0 - 5.0
    for pad, off in RED_LD:
        for det in (False, True):
            ey, ecen = embed(Y, _ld(D, pad), off, dev), _vec(centre, dev)
            s1, s2 = _vec(s0, dev), _vec(s0, dev)
            _lib.call("pm_col_moments_f64", ey.ptr, ey.ld, N, D, None, s1.ptr, _stream(), det=det)
            _lib.call("pm_col_moments_f64", ey.ptr, ey.ld, N, D, ecen.ptr, s2.ptr, _stream(), det=det)
            torch.cuda.synchronize()
            assert np.array_equal(s1.block().cpu().numpy()[0], s0 + Y.sum(0)), (pad, off, det)
            assert np.array_equal(s2.block().cpu().numpy()[0], s0 + ((Y - centre) ** 2).sum(0)), (pad, off, det)
            assert s1.outside_untouched() and s2.outside_untouched() and ey.unchanged() and ecen.unchanged()


@pytest.mark.parametrize("N", RED_N)
@pytest.mark.parametrize("D", RED_D)
def test_col_sum_kept(dev, det_quanta, D, N):
    """pm_col_sum_kept_f64: rows with lse >= cut are summed -- entries EQUAL to the cut are kept, a NaN and a -inf are
    dropped; cut = -inf keeps everything but the NaN; `sums` is accumulated into."""
    from prosper_amd import _lib
    Y, s0 = ints(N, D, 3 * N + D), np.arange(D) * 3.0 + 1.0
    cut = 0.5
    lse = np.random.RandomState(N * D).choice([cut, cut + 1.0, cut - 1.0, cut], size=N)
    if N >= 3:
        lse[N // 2], lse[N - 1], lse[0] = np.nan, -np.inf, cut
    assert (lse == cut).any() or N < 3
    for c in (cut, -np.inf):
        with np.errstate(invalid="ignore"):
            keep = lse >= c
        ref = s0 + Y[keep].sum(0)
        for pad, off in RED_LD:
            for det in (False, True):
                ey, el, s = embed(Y, _ld(D, pad), off, dev), _vec(lse, dev), _vec(s0, dev)
                _lib.call("pm_col_sum_kept_f64", ey.ptr, ey.ld, N, D, el.ptr, ctypes.c_double(c), s.ptr, _stream(), det=det)
                torch.cuda.synchronize()
                assert np.array_equal(s.block().cpu().numpy()[0], ref), (c, pad, off, det)
                assert s.outside_untouched() and ey.unchanged() and el.unchanged()


# ------------------------------------------------------------------------------------------------ rounding bound
def _rows_subset(M, rng, n=96):
    """All rows of a small product; of a tall one the first and last 24 and a seeded draw between them."""
    if M <= 2 * n:
        return np.arange(M)
    return np.unique(np.concatenate([np.arange(24), np.arange(M - 24, M), rng.randint(24, M - 24, size=n - 48)]))


def _rounding_cases():
    c = []
    for name in ("main", "fused", "rest64", "rest", "mt1_al", "mt1_un", "mt2_un", "mt2_al", "mt4_un", "mt4_al"):
        c.append(("pm_gemm_nt_f64", name, False))
    c += [("pm_gemm_nt_f64", "fused", True), ("pm_gemm_nt_f64", (130, 128, 512), False),      # (split-K: 8 slices of 8 K-steps)
          ("pm_gemm_nt_rows_f64", (200, 144, 64), False), ("pm_gemm_nt_rows_f64", (200, 144, 50), False),
          ("pm_gemm_nt_small_f64", (100, 37, 1040), False), ("pm_gemm_nt_small_f64", (100, 37, 25), False),
          ("pm_gemm_nn_small_f64", (20, 33, 1040), False), ("pm_gemm_nn_small_f64", (20, 33, 18), False),
          ("pm_gemm_tn_acc_f64", (128, 128, 2055), False), ("pm_gemm_tn_acc_f64", (130, 128, 1024), False),
          ("pm_gemm_tn_acc_f64", (33, 7, 333), False), ("pm_gemm_tn_acc_gated_f64", (128, 128, 71), False),
          ("pm_gemm_tn_acc_rows_f64", (128, 128, 200), False)]
    return c


@pytest.mark.parametrize("entry,shape,det", _rounding_cases(),
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_rounding_bound(dev, slots, entry, shape, det):
    """Standard-normal operands, one shape per kernel family, against an 80-bit reference (on the rows of ``_rows_subset``
    for the tall shapes): the componentwise bound of a length-K inner product in any summation order, K products and at
    most K additions each within 2^-53 relative -- (K + 2) 2^-53 (|A| |B|^T), and (K + 3) 2^-53 (|A|^T |B| + |C0|) for
    the forms that add to C.  Not widened by any measurement."""
    from prosper_amd import _lib
    M, N, K = nt_path_cases(slots)[shape][:3] if isinstance(shape, str) else shape
    rng = np.random.RandomState(M + 3 * N + 5 * K)
    st = _stream()
    if "_tn_" in entry:
        A, B, C0 = rng.normal(size=(K, M)), rng.normal(size=(K, N)), rng.normal(size=(M, N))
        if entry == "pm_gemm_tn_acc_rows_f64":
            A[K - 1] = B[K - 1] = 0.0            # the zero row
        a, b, c = (_t(x).to(dev) for x in (A, B, C0))
        if entry == "pm_gemm_tn_acc_rows_f64":
            rows = rng.permutation(K - 1)[:K - 9].astype(np.int32)
            r, n = torch.from_numpy(rows).to(dev), torch.tensor([len(rows)], dtype=torch.int32, device=dev)
            _lib.call(entry, a.data_ptr(), M, b.data_ptr(), N, c.data_ptr(), N, M, N, r.data_ptr(), n.data_ptr(), K, K - 1, st)
            A, B = A[rows], B[rows]
        elif entry == "pm_gemm_tn_acc_gated_f64":
            g = torch.ones(1, dtype=torch.float64, device=dev)
            _lib.call(entry, a.data_ptr(), M, b.data_ptr(), N, c.data_ptr(), N, M, N, K, g.data_ptr(), st)
        else:
            _lib.call(entry, a.data_ptr(), M, b.data_ptr(), N, c.data_ptr(), N, M, N, K, st)
        got = c.cpu().numpy()
        ref = C0.astype(np.longdouble) + _matmul_hi(A.T, B)
        bound = (A.shape[0] + 3) * U * (np.abs(A).T @ np.abs(B) + np.abs(C0))
    else:
        nn = entry == "pm_gemm_nn_small_f64"
        A, B = rng.normal(size=(M, K)), rng.normal(size=(K, N) if nn else (N, K))
        a, b = _t(A).to(dev), _t(B).to(dev)
        c = torch.full((M, N), float("nan"), dtype=torch.float64, device=dev)
        _lib.call(entry, a.data_ptr(), K, b.data_ptr(), N if nn else K, c.data_ptr(), N, M, N, K, st, det=det)
        sub = _rows_subset(M, rng)
        got = c[torch.from_numpy(sub).to(dev)].cpu().numpy()
        Bt = B if nn else B.T
        ref = _matmul_hi(A[sub], Bt)
        bound = (K + 2) * U * (np.abs(A[sub]) @ np.abs(Bt))
    assert not np.isnan(got).any()
    err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    worst = float((err / bound).max())
    print("%s %s: max |C - Chat| / bound = %.3g" % (entry, (M, N, K), worst))
    assert (err <= bound).all(), worst
