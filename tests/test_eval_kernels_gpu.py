"""The evaluation kernels (masked_kernels.hip, reconstruct_kernels.hip) through the C ABI -- pm_masked_prepare_f64,
pm_bsc_masked_estep_f64, pm_mca_masked_select_scores_f64, pm_mca_masked_estep_f64, pm_recon_expect_f64, pm_recon_mca_f64 -- on
padded operands, at every template instantiation and tile edge, EXACTLY wherever the arithmetic allows it.

Harness (the method of tests/test_dense_kernels_gpu.py, for three element types).  ``Emb`` places every operand and every
output inside a larger device buffer filled with one recognisable pattern (f64: a quiet NaN with a payload no arithmetic
produces; int32: 0xDEADBEEF; uint8: 0xA5, a NON-ZERO byte -- a mask byte read past a row's D columns reads "observed"): 16
guard rows of ``ld`` elements before and after and the padding columns [width, ld) of every row.  After a call the result
block is compared, every other element of an output buffer must still hold the pattern, and the inputs must be bit-unchanged.
Leading dimensions: tight, the smallest even and the smallest odd stride with padding, and two mixtures that give
neighbouring operands different ones (``LAYOUTS``).  The uint8 mask starts at an odd byte address in every layout.

Exact arithmetic.  Data, weights and means are small integers wherever a kernel only adds and multiplies: every partial sum
is an integer far below 2^53, any summation order gives NumPy's bits, and the comparison is equality (prepare, the MCA
selection scores, the BSC candidates and energies).  The BSC scores b / sqrt(g) are exact for perfect-square g (sqrt and the
division are correctly rounded on both sides), so ties are real ties.  BSC log-joints ppil |s| + ecoef e: e is exact, the
two products and the sum round -- two roundings, or one with a fused multiply-add -- so 4 ulp of the larger term bounds any
correct evaluation.  Where a kernel calls its power functions or exp (MCA energies, the posterior weights) the bound is the
modules' 1e-11 row-relative (tests/test_masked_gpu.py, tests/test_reconstruct_gpu.py).

NumPy references: tests/masked_reference.py (bsc_select_rule, bsc_masked_terms) and tests/recon_reference.py (expect_from_lpj,
mca_multi_from_lpj), pinned on the CPU by tests/test_masked_cpu.py and tests/test_reconstruct_cpu.py."""
import ctypes

import numpy as np
import pytest
from scipy.special import logsumexp

import masked_reference as MR
import recon_reference as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT_F64 = 0x7FF8DEADBEEF0001
SENT_I32 = -559038737                  # 0xDEADBEEF
SENT_U8 = 0xA5
GUARD_ROWS = 16
RTOL = 1e-11
LAYOUTS = ["tight", "even", "odd", "mix_a", "mix_b"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs the GPU box (MI355X)")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ld(width, layout, k):
    """Leading dimension of the k-th operand of a call in ``layout``."""
    kind = {"tight": "t", "even": "e", "odd": "o", "mix_a": "teo"[k % 3], "mix_b": "ote"[k % 3]}[layout]
    if kind == "t":
        return width
    return width + 1 + ((width + 1) % 2 if kind == "e" else width % 2)


class Emb:
    """A host matrix (or vector: one row) of float64, int32 or uint8 inside a pattern-filled device buffer."""
    _TYPES = {np.dtype(np.float64): (torch.float64, SENT_F64), np.dtype(np.int32): (torch.int32, SENT_I32),
              np.dtype(np.uint8): (torch.uint8, SENT_U8)}

    def __init__(self, array, ld, dev, off=0, fill=True):
        a = np.asarray(array)
        a = a[None, :] if a.ndim == 1 else a
        self.rows, self.cols = a.shape
        assert ld >= self.cols
        self.ld = ld
        tdt, self.sent = self._TYPES[a.dtype]
        self.item = a.dtype.itemsize
        self.start = GUARD_ROWS * ld + off
        self.buf = torch.empty(self.start + (self.rows + GUARD_ROWS) * ld + 3, dtype=tdt, device=dev)
        self._raw().fill_(self.sent)
        if fill and a.size:
            self.block().copy_(torch.from_numpy(np.ascontiguousarray(a)))
        self.before = self.buf.clone()

    def _raw(self, t=None):
        t = self.buf if t is None else t
        return t.view(torch.int64) if t.dtype == torch.float64 else t

    def block(self):
        return self.buf[self.start:self.start + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols]

    def host(self):
        return self.block().cpu().numpy()

    @property
    def addr(self):
        return self.buf.data_ptr() + self.item * self.start

    @property
    def ptr(self):
        return ctypes.c_void_p(self.addr)

    def unchanged(self):
        return torch.equal(self._raw(), self._raw(self.before))

    def outside_untouched(self):
        rest = self._raw().clone()
        rest[self.start:self.start + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols] = self.sent
        return bool((rest == self.sent).all())

    def written(self):
        """No element of the result block still holds the pattern."""
        return not bool((self._raw()[self.start:self.start + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols]
                         == self.sent).any())


def emb_mask(M, ld, dev):
    """The uint8 mask at an ODD byte address (the buffer's base is 16-byte aligned)."""
    e = Emb(M, ld, dev, off=1 if (GUARD_ROWS * ld) % 2 == 0 else 2)
    assert e.addr % 2 == 1
    return e


def ints(rows, cols, seed, lo=-8, hi=8):
    """Position-dependent integers in [lo, hi] as f64 (not symmetric: a transposed or shifted tile map changes the answer)."""
    rng = np.random.RandomState(seed)
    i, j = np.arange(rows)[:, None], np.arange(cols)[None, :]
    return (lo + (rng.randint(0, hi - lo + 1, size=(rows, cols)) + (i + 3 * j) % 5) % (hi - lo + 1)).astype(np.float64)


def mask_bytes(N, D, seed, frac=0.6):
    """Observed entries carry 1, 200 or 255 (any non-zero byte means observed); row 0 fully observed, the last row not at all
    (when there are at least three)."""
    rng = np.random.RandomState(seed)
    M = (rng.uniform(size=(N, D)) < frac) * rng.choice([1, 200, 255], size=(N, D))
    if N >= 3:
        M[0] = np.where(M[0] == 0, 7, M[0])
        M[N - 1] = 0
    return M.astype(np.uint8)


def garbage(Y, M, seed):
    """Y with NaN, +inf, -inf and 1e300 at the unobserved entries."""
    rng = np.random.RandomState(seed)
    junk = rng.choice([np.nan, np.inf, -np.inf, 1e300], size=Y.shape)
    return np.where(M != 0, Y, junk)


def row_rel(got, want):
    scale = np.abs(want).max(axis=1)
    return float((np.abs(got - want).max(axis=1) / np.where(scale > 0, scale, 1.0)).max())


def _ok(*embs):
    return all(e.unchanged() for e in embs)


# ------------------------------------------------------------------------------------------------ pm_masked_prepare_f64
@pytest.mark.parametrize("D", [1, 63, 64, 65, 130])
def test_masked_prepare(dev, D):
    """X0 = m ? y - mu : 0, Mf = m ? 1 : 0, D_n and (integer data) |X0|^2 equal NumPy; with and without mu and Mf; N = 8197
    rows of D <= 3 reach the second trip of the row loop (2048 workgroups of four rows)."""
    from prosper_amd import _lib
    for N in (1, 5, 70) + ((8197,) if D == 1 else ()):
        Y0, M = ints(N, D, N + D), mask_bytes(N, D, N * D)
        Y = garbage(Y0, M, N + 2 * D)
        for with_mu in (False, True):
            mu = ints(1, D, D + 5, -3, 3)[0] if with_mu else None
            X0 = np.where(M != 0, Y0 - (mu if with_mu else 0.0), 0.0)
            for layout in LAYOUTS:
                for with_mf in (True, False):
                    ey, em = Emb(Y, _ld(D, layout, 0), dev), emb_mask(M, _ld(D, layout, 1), dev)
                    emu = Emb(mu, D, dev) if with_mu else None
                    ex = Emb(X0, _ld(D, layout, 2), dev, fill=False)
                    ef = Emb(X0, _ld(D, layout, 3), dev, fill=False)
                    en, ed = Emb(np.zeros(N), N, dev, fill=False), Emb(np.zeros(N, dtype=np.int32), N, dev, fill=False)
                    _lib.call("pm_masked_prepare_f64", ey.ptr, ey.ld, em.ptr, em.ld, emu.ptr if with_mu else None, N, D,
                              ex.ptr, ex.ld, ef.ptr if with_mf else None, ef.ld, en.ptr, ed.ptr, _stream())
                    torch.cuda.synchronize()
                    what = (N, D, with_mu, layout, with_mf)
                    assert np.array_equal(ex.host(), X0), what
                    assert np.array_equal(en.host()[0], (X0 * X0).sum(axis=1)), what
                    assert np.array_equal(ed.host()[0], (M != 0).sum(axis=1)), what
                    if with_mf:
                        assert np.array_equal(ef.host(), (M != 0).astype(np.float64)), what
                    else:
                        assert ef.unchanged(), what
                    assert ex.outside_untouched() and ef.outside_untouched() and en.outside_untouched() \
                        and ed.outside_untouched(), what
                    assert _ok(ey, em) and (emu is None or emu.unchanged()), what


# ------------------------------------------------------------------------------------- pm_mca_masked_select_scores_f64
@pytest.mark.parametrize("H", [1, 63, 64, 65, 130])
def test_mca_masked_select_scores(dev, H):
    """R[n,h] = sum_d m_d max(W[h,d] - y_d, 0): one thread adds fmax(w - y, 0) in ascending d, on integers exact in any
    order.  64 x 64 output tiles: H and N of 1, 63, 64, 65 and 130 (three H tiles with a ragged last one), D across the
    16-wide slabs.  Whatever the unobserved entries hold (NaN, +-inf, 1e300, or 0) changes no bit."""
    from prosper_amd import _lib
    for N in (1, 63, 65):
        for D in (1, 15, 16, 17, 70):
            Y0, W, M = ints(N, D, N + D), ints(H, D, H + 3 * D + 1), mask_bytes(N, D, N + H + D)
            want = np.where((M != 0)[:, None, :], np.maximum(W[None, :, :] - Y0[:, None, :], 0.0), 0.0).sum(axis=2)
            for k, layout in enumerate(LAYOUTS):
                Y = garbage(Y0, M, k) if k else np.where(M != 0, Y0, 0.0)
                ey, em = Emb(Y, _ld(D, layout, 0), dev), emb_mask(M, _ld(D, layout, 1), dev)
                ew, er = Emb(W, _ld(D, layout, 2), dev), Emb(want, _ld(H, layout, 3), dev, fill=False)
                _lib.call("pm_mca_masked_select_scores_f64", ey.ptr, ey.ld, em.ptr, em.ld, ew.ptr, ew.ld, er.ptr, er.ld, N, H,
                          D, _stream())
                torch.cuda.synchronize()
                got = er.host()
                assert np.array_equal(got, want), (N, H, D, layout, np.argwhere(got != want)[:5].tolist())
                assert er.outside_untouched() and _ok(ey, em, ew), (N, H, D, layout)


# --------------------------------------------------------------------------------------------- pm_bsc_masked_estep_f64
def _bsc_model(D, H, Hp, g):
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels._device import LoglikPoint
    m = BSC_ET(D, H, Hp, g)
    P = m._estep_params(LoglikPoint(), 0.1, 1.3, np.zeros(1))          # the library's struct, filled by the model itself
    return m, P


def _run_bsc(dev, m, P, b, g, xn2, M, Wt, layout):
    """One call on embedded operands; returns (cand, logpj) after the sentinel and input checks."""
    from prosper_amd import _lib
    N, H = b.shape
    D, Hp, S = Wt.shape[1], m.Hprime, m.no_states
    K = 1 + H + S
    eb, eg = Emb(b, _ld(H, layout, 0), dev), Emb(g, _ld(H, layout, 1), dev)
    en, em, ew = Emb(xn2, N, dev), emb_mask(M, _ld(D, layout, 2), dev), Emb(Wt, _ld(D, layout, 3), dev)
    ec = Emb(np.zeros((N, Hp), dtype=np.int32), Hp, dev, fill=False)
    el = Emb(np.zeros((N, K)), _ld(K, layout, 4), dev, fill=False)
    masks = m._state_tables()["masks"]
    _lib.call("pm_bsc_masked_estep_f64", eb.ptr, eb.ld, eg.ptr, eg.ld, en.ptr, em.ptr, em.ld, ew.ptr, ew.ld,
              ctypes.c_void_p(masks.data_ptr()), S, ctypes.byref(P), N, H, D, Hp, ec.ptr, el.ptr, el.ld, _stream())
    torch.cuda.synchronize()
    what = (H, D, Hp, layout)
    assert ec.outside_untouched() and el.outside_untouched(), what
    assert ec.written() and _ok(eb, eg, en, em, ew), what
    return ec.host(), el.host()


def _check_bsc_logpj(P, m, b, g, xn2, M, Wt, cand, got, rows, what):
    """logpj = ppil |s| + ecoef e with e exact: 4 ulp of the larger term."""
    ppil = P.prior_scale * P.pil_bar
    size, e = MR.bsc_masked_terms(b[rows], g[rows], xn2[rows], M[rows], Wt, cand[rows], m.state_matrix)
    t1, t2 = ppil * size, P.ecoef * e
    bound = 4 * np.spacing(np.maximum(np.abs(t1), np.abs(t2)))
    err = np.abs(got[rows] - (t1 + t2))
    assert np.isfinite(got[rows]).all(), what
    assert (err <= bound).all(), (what, float((err / np.where(bound > 0, bound, 1.0)).max()))


# (H, D, H', gamma): one H per latents-per-lane instantiation (VPL 1, 2, 4, 8, 16: H <= 64 VPL, PM_MAX_H = 1024 itself), H'
# of 12 and 16 -- 66 and 120 candidate pairs, the second pair of a lane --, D below, at and across the 64-wide slabs
BSC_SHAPES = [(61, 70, 5, 3), (125, 33, 12, 2), (253, 64, 6, 3), (509, 130, 5, 2), (1024, 40, 16, 2)]


@pytest.mark.parametrize("H,D,Hp,gamma", BSC_SHAPES)
def test_bsc_masked_estep_integer_data(dev, H, D, Hp, gamma):
    """b, diag G_n and |x|^2 formed exactly in NumPy from integer data: the candidates equal the selection rule on the
    exact scores, the energies are exact, the log-joints within 4 ulp, in every layout."""
    N = 9
    m, P = _bsc_model(D, H, Hp, gamma)
    X, M, Wt = ints(N, D, H + D), mask_bytes(N, D, H * D), ints(H, D, 7 * H + D, -3, 3)
    Mf = (M != 0).astype(np.float64)
    X0 = np.where(M != 0, X, 0.0)
    b, g, xn2 = X0 @ Wt.T, Mf @ (Wt * Wt).T, (X0 * X0).sum(axis=1)
    want_c = MR.bsc_select_rule(b, g, Hp)
    for layout in LAYOUTS:
        cand, logpj = _run_bsc(dev, m, P, b, g, xn2, M, Wt, layout)
        assert np.array_equal(cand, want_c), (H, layout, np.argwhere(cand != want_c)[:5].tolist())
        _check_bsc_logpj(P, m, b, g, xn2, M, Wt, cand, logpj, np.arange(N), (H, D, Hp, layout))


@pytest.mark.parametrize("H,D,Hp,gamma", BSC_SHAPES)
def test_bsc_masked_estep_tie_rule(dev, H, D, Hp, gamma):
    """b and g given directly, g of perfect squares: real ties at the selection boundary -- between two lanes, between two
    slots of one lane (h and h + 64; h and h + 64 (VPL - 1)), between a g = 0 latent and a true zero score --, NaN scores,
    and rows where more than H - H' scores are -inf.  "The H' largest, ascending, ties towards the larger index"."""
    vpl = (H + 63) // 64
    m, P = _bsc_model(D, H, Hp, gamma)
    rng = np.random.RandomState(H)
    M, Wt = mask_bytes(10, D, H + 1), ints(H, D, 3 * H + D, -3, 3)
    N = 10
    b = -(10.0 + rng.randint(0, 40, size=(N, H)))           # background: scores in [-49, -10], full of ties below the cut
    g = np.ones((N, H))
    pool = np.setdiff1d(np.arange(H // 2, H), [5, 9, 7, 7 + 64, 7 + 64 * (vpl - 1), 11, 13, 20, 3, 40])
    top = rng.permutation(pool)[:Hp - 1]                     # H' - 1 clear winners: one place left for the tie
    for n in range(N):
        b[n, top] = 100.0 + np.arange(len(top))
    pairs = {}
    # 1: two lanes, 6 / sqrt(4) == 9 / sqrt(9) == 3
    b[1, [5, 9]], g[1, [5, 9]] = (6.0, 9.0), (4.0, 9.0)
    pairs[1] = (5, 9)
    if vpl >= 2:        # 2, 3: two slots of lane 7
        for n, hi in ((2, 7 + 64), (3, 7 + 64 * (vpl - 1))):
            if hi < H:
                b[n, [7, hi]], g[n, [7, hi]] = (2.0, 4.0), (9.0, 36.0)      # 2 / 3 == 4 / 6, one rounding of the same rational
                pairs[n] = (7, hi)
    # 4: a latent nothing observed supports (g = 0: score 0 whatever b holds) against a true zero (b = 0, g = 4)
    b[4, [11, 13]], g[4, [11, 13]] = (123.0, 0.0), (0.0, 4.0)
    pairs[4] = (11, 13)
    # 5: the order of the two reversed
    b[5, [11, 13]], g[5, [11, 13]] = (0.0, 25.0), (-77.0, 0.0)
    pairs[5] = (11, 13)
    # 6: NaN scores where the largest would be: they rank lowest
    b[6, top[:1]] = np.nan
    b[6, 20] = np.nan
    # 7: all but two scores NaN, 8: all but two -inf, 9: every score -inf -- the largest indices fill the list
    b[7], b[8], b[9] = np.nan, -np.inf, -np.inf
    b[7, [3, 40]], b[8, [3, 40]] = (-5.0, -6.0), (-5.0, -6.0)
    want_c = MR.bsc_select_rule(b, g, Hp)
    # the scenarios are what they claim to be (on the reference)
    for n, (lo, hi) in pairs.items():
        assert hi in want_c[n] and lo not in want_c[n], (n, want_c[n])
    assert not np.isin(want_c[6], [top[0], 20]).any()
    assert np.array_equal(want_c[9], np.arange(H - Hp, H)) and {3, 40} <= set(want_c[7]) and {3, 40} <= set(want_c[8])
    assert np.array_equal(want_c[7][:-2] if Hp > 2 else [], np.sort(np.setdiff1d(np.arange(H), [3, 40])[-(Hp - 2):]) if Hp > 2 else [])
    xn2 = np.arange(N) + 50.0
    finite = np.array([n for n in range(N) if np.isfinite(b[n]).all()])
    for layout in ("tight", "odd", "mix_a"):
        cand, logpj = _run_bsc(dev, m, P, b, g, xn2, M, Wt, layout)
        assert np.array_equal(cand, want_c), (H, layout, [(n, cand[n].tolist(), want_c[n].tolist())
                                                          for n in range(N) if not np.array_equal(cand[n], want_c[n])])
        _check_bsc_logpj(P, m, b, g, xn2, M, Wt, cand, logpj, finite, (H, D, Hp, layout))


# ------------------------------------------------------------------------- pm_mca_masked_estep_f64 / pm_recon_mca_f64
def _mca_model(D, H, Hp, g, signed):
    from prosper_amd.em.camodels.mca_et import MCA_ET
    from prosper_amd.em.camodels.mmca_et import MMCA_ET
    return (MMCA_ET if signed else MCA_ET)(D, H, Hp, g)


def _mca_weights(H, D, rho, signed, seed):
    rng = np.random.RandomState(seed)
    W = rng.uniform(0.1, 3.0, size=(H, D))
    if signed:
        W = W * rng.choice([-1.0, 1.0], size=(H, D))
    return W, np.sign(W) * np.abs(W) ** rho


# (D, rho, signed): one D per dimensions-per-lane instantiation (DPL 1, 2, 4, 8, 16), each reaching the lane's LAST slab of 64
# dimensions (D > 64 (DPL - 1)), and one D that fills it (256); the two special roots and a general one
MCA_SHAPES = [(40, 21.0, False), (100, 6.0, True), (200, 3.5, False), (500, 3.5, True), (1000, 21.0, False), (256, 6.0, True)]


@pytest.mark.parametrize("D,rho,signed", MCA_SHAPES)
def test_mca_masked_estep(dev, D, rho, signed):
    """[null ; H one-cause ; S multi-cause] log-joints and the two row log-sum-exps (beta = 0.8) against NumPy at 1e-11
    row-relative; padded lds / ldwn / ldx / ldm / ldl."""
    from prosper_amd import _lib
    H, Hp, gam, N = 20, 5, 2, 9
    m = _mca_model(D, H, Hp, gam, signed)
    P = m._params({"T": 1.25}, 0.1, 0.9, rho)
    S = m.no_states
    K = 1 + H + S
    Wt, Wrho = _mca_weights(H, D, rho, signed, D)
    rng = np.random.RandomState(D + 1)
    M = mask_bytes(N, D, D + 2)
    Mb = M != 0
    X0 = np.where(Mb, rng.uniform(-1 if signed else 0, 3, size=(N, D)), 0.0)
    A, wn, xn2 = X0 @ Wt.T, Mb.astype(np.float64) @ (Wt * Wt).T, (X0 * X0).sum(axis=1)
    cand = np.array([rng.permutation(H)[:Hp] for _ in range(N)], dtype=np.int32)
    SM = np.asarray(m.state_matrix) != 0
    want = np.empty((N, K))
    want[:, 0] = P.pre1 * xn2
    want[:, 1:1 + H] = P.pil_bar + P.pre1 * (wn - 2.0 * A + xn2[:, None])
    for n in range(N):
        for s, row in enumerate(SM):
            T = Wrho[cand[n, row]].sum(axis=0)
            wbar = np.sign(T) * np.abs(T) ** (1. / rho)
            want[n, 1 + H + s] = P.pil_bar * row.sum() + P.pre1 * (np.where(Mb[n], wbar - X0[n], 0.0) ** 2).sum()
    masks = m._u16_dev(m._state_masks())
    for layout in LAYOUTS:
        ea, ewn = Emb(A, _ld(H, layout, 0), dev), Emb(wn, _ld(H, layout, 1), dev)
        en, ex, em = Emb(xn2, N, dev), Emb(X0, _ld(D, layout, 2), dev), emb_mask(M, _ld(D, layout, 3), dev)
        ewr, ec = Emb(Wrho, D, dev), Emb(cand, Hp, dev)
        el = Emb(want, _ld(K, layout, 4), dev, fill=False)
        e1, eb = Emb(np.zeros(N), N, dev, fill=False), Emb(np.zeros(N), N, dev, fill=False)
        _lib.call("pm_mca_masked_estep_f64", ea.ptr, ea.ld, ewn.ptr, ewn.ld, en.ptr, ex.ptr, ex.ld, em.ptr, em.ld, ewr.ptr,
                  ec.ptr, ctypes.c_void_p(masks.data_ptr()), S, ctypes.byref(P), N, H, D, Hp, el.ptr, el.ld, e1.ptr, eb.ptr,
                  _stream())
        torch.cuda.synchronize()
        got = el.host()
        err = row_rel(got, want)
        print("pm_mca_masked_estep_f64 D=%d rho=%g signed=%d %-6s row-relative error %.3e" % (D, rho, signed, layout, err))
        assert np.isfinite(got).all() and err <= RTOL, (D, rho, layout, err)
        np.testing.assert_allclose(e1.host()[0], logsumexp(want, axis=1), rtol=RTOL)
        np.testing.assert_allclose(eb.host()[0], logsumexp(P.beta * want, axis=1), rtol=RTOL)
        assert el.outside_untouched() and e1.outside_untouched() and eb.outside_untouched(), (D, layout)
        assert _ok(ea, ewn, en, ex, em, ewr, ec), (D, layout)


@pytest.mark.parametrize("D,rho,signed", MCA_SHAPES)
def test_recon_mca(dev, D, rho, signed):
    """Yhat += sum_s q_s Wbar(s) into a NON-ZERO Yhat with a padded row: the sum is Yhat0 plus NumPy's increment at 1e-11
    row-relative, columns >= D of every row keep the pattern; the row log-sum-exp given and formed by the kernel."""
    from prosper_amd import _lib
    H, Hp, gam, N = 20, 5, 2, 9
    m = _mca_model(D, H, Hp, gam, signed)
    S = m.no_states
    K = 1 + H + S
    _, Wrho = _mca_weights(H, D, rho, signed, D + 7)
    rng = np.random.RandomState(D + 3)
    lp = 2.0 * rng.normal(size=(N, K))
    lse = logsumexp(lp, axis=1)
    cand = np.array([rng.permutation(H)[:Hp] for _ in range(N)], dtype=np.int32)
    Y0 = rng.normal(size=(N, D))
    inc = R.mca_multi_from_lpj(lp, lse, cand, m.state_matrix, Wrho, rho, signed)
    assert np.abs(inc).max() > 0.1          # (the increment is of the size of Yhat0: the comparison sees it)
    want = Y0 + inc
    masks = m._u16_dev(m._state_masks())
    for layout in LAYOUTS:
        for given in (False, True):
            el, els = Emb(lp, _ld(K, layout, 0), dev), Emb(lse, N, dev)
            ec, ewr = Emb(cand, Hp, dev), Emb(Wrho, D, dev)
            ey = Emb(Y0, _ld(D, layout, 1) if layout != "tight" or given else D + 3, dev)
            _lib.call("pm_recon_mca_f64", el.ptr, el.ld, els.ptr if given else None, ec.ptr, ctypes.c_void_p(masks.data_ptr()),
                      ewr.ptr, ctypes.c_double(1. / rho), int(signed), N, H, D, Hp, S, ey.ptr, ey.ld, _stream())
            torch.cuda.synchronize()
            err = row_rel(ey.host(), want)
            print("pm_recon_mca_f64 D=%d rho=%g signed=%d %-6s lse %s row-relative error %.3e" % (
                D, rho, signed, layout, "given" if given else "formed", err))
            assert err <= RTOL, (D, rho, layout, given, err)
            assert ey.outside_untouched() and _ok(el, els, ec, ewr), (D, layout, given)


# -------------------------------------------------------------------------------------------------- pm_recon_expect_f64
def _run_expect(dev, X, a, off, cand, table, blocks, H, soff, moff, out_cols, ones_col, layout, lse=None):
    from prosper_amd import _lib
    N, K = X.shape
    S = 0 if table is None else table.shape[0]
    Hp = 0 if table is None else table.shape[1]
    ex = Emb(X, _ld(K, layout, 0) if layout != "tight" else K + 5, dev)          # ld > K in every layout
    eo = Emb(np.zeros((N, out_cols)), _ld(out_cols, layout, 1) if layout != "tight" else out_cols + 3, dev, fill=False)
    eoff = Emb(off, K, dev) if off is not None else None
    elw = Emb(lse, N, dev) if lse is not None else None
    ec = Emb(np.asarray(cand, dtype=np.int32), Hp, dev) if S else None
    et = Emb(np.asarray(table, dtype=np.float64), Hp, dev) if S else None
    bv = (ctypes.c_double * 8)(*([float(v) for v in blocks] + [0.0] * (8 - len(blocks))))
    _lib.call("pm_recon_expect_f64", ex.ptr, ex.ld, elw.ptr if elw else None, ctypes.c_double(a),
              eoff.ptr if eoff else None, ec.ptr if S else None, et.ptr if S else None, bv, N, H, Hp, K, soff, len(blocks), moff,
              S, eo.ptr, eo.ld, out_cols, ones_col, _stream())
    torch.cuda.synchronize()
    assert eo.ld > out_cols and ex.ld > K
    assert eo.outside_untouched(), "a column past out_cols or a guard row was written"
    assert all(e.unchanged() for e in (ex, eoff, elw, ec, et) if e is not None)
    got = eo.host()
    want = R.expect_from_lpj(X, a, cand, H, blocks, soff, moff, table, off=off)
    tail = np.zeros((N, out_cols - H))
    if ones_col >= 0:
        tail[:, ones_col - H] = 1.0
    assert np.array_equal(got[:, H:], tail), "columns [H, out_cols) are 0 except the column of ones"
    return got[:, :H], want


def _table_states(Hp, gamma, values, rng):
    from prosper_amd.em.camodels import generate_state_matrix
    SM = np.asarray(generate_state_matrix(Hp, gamma)[2], dtype=np.float64)
    return SM * rng.choice(values, size=SM.shape)


@pytest.mark.parametrize("layout", ["tight", "even", "odd"])
def test_recon_expect(dev, layout):
    """E[s] of the linear models and the normalised weights of a mixture against NumPy at 1e-11 row-relative; ld > K and
    ldo > out_cols everywhere; the tail columns exact."""
    rng = np.random.RandomState(len(layout))
    N = 11
    # BSC layout: [null ; H ; S], one block of value 1, H = 70 > 64 (the lane-strided loop), H' = 12; a column of ones at H;
    # lse formed by the kernel and given
    H, Hp = 70, 12
    tab = _table_states(Hp, 2, [1.0], rng)
    K = 1 + H + len(tab)
    X = 3.0 * rng.normal(size=(N, K))
    cand = np.array([np.sort(rng.permutation(H)[:Hp]) for _ in range(N)])
    for lse in (None, logsumexp(X, axis=1)):
        got, want = _run_expect(dev, X, 1.0, None, cand, tab, (1.0,), H, 1, 1 + H, 72, H, layout, lse=lse)
        err = row_rel(got, want)
        print("pm_recon_expect_f64 bsc layout %-5s lse %s: %.3e" % (layout, "formed" if lse is None else "given", err))
        assert err <= RTOL, err
    # DSC layout with 8 latent values: nblk = 7 blocks of H = 70 columns, H' = 16 (PM_MAX_HPRIME), no column of ones
    vals = (-3., -2., -1., 1., 2., 3., 4.)
    tab = _table_states(16, 2, vals, rng)
    K = 1 + 7 * H + len(tab)
    X = 3.0 * rng.normal(size=(N, K))
    cand = np.array([np.sort(rng.permutation(H)[:16]) for _ in range(N)])
    got, want = _run_expect(dev, X, 1.0, None, cand, tab, vals, H, 1, 1 + 7 * H, 77, -1, layout)
    err = row_rel(got, want)
    print("pm_recon_expect_f64 dsc8 layout %-5s: %.3e" % (layout, err))
    assert err <= RTOL, err
    # TSC layout: table states only, values -1 / +1, rows whose candidates repeat a latent: both positions' sums
    Hp = 5
    tab = _table_states(Hp, 3, [-1.0, 1.0], rng)
    X = 3.0 * rng.normal(size=(N, len(tab)))
    cand = np.array([rng.permutation(H)[:Hp] for _ in range(N)])
    cand[2, 3] = cand[2, 0]
    cand[5, 4] = cand[5, 1] = cand[5, 2]
    cand[7, :] = 69
    got, want = _run_expect(dev, X, 1.0, None, cand, tab, (), H, 0, 0, 72, 71, layout)
    err = row_rel(got, want)
    print("pm_recon_expect_f64 tsc layout %-5s: %.3e" % (layout, err))
    assert err <= RTOL, err
    assert np.abs(want[7, :69]).max() == 0.0 and abs(want[7, 69]) > 0     # (all five positions land on latent 69)
    # mixture use: a != 1 with a column offset, no candidates, no table; the column of ones absent, at H, at out_cols - 1
    H = 21
    X, off = 3.0 * rng.normal(size=(N, H)), rng.normal(size=H)
    for out_cols, ones_col in ((H, -1), (24, H), (24, 23)):
        got, want = _run_expect(dev, X, 0.7, off, None, None, (1.0,), H, 0, 0, out_cols, ones_col, layout)
        err = row_rel(got, want)
        print("pm_recon_expect_f64 mixture layout %-5s ones_col %d: %.3e" % (layout, ones_col, err))
        assert err <= RTOL, err
        np.testing.assert_allclose(got.sum(axis=1), 1.0, rtol=1e-12)
