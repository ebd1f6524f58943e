"""reconstruct_image() / utils.patches without a GPU: the NumPy reference the GPU tests compare against
(tests/patches_reference.py) pins itself, the package's grid rule is the reference's, argument errors are raised before any
device call, and the pm_patches_* entries exist in the header, the binding and both libraries and reject bad arguments
before they touch a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import patches_reference as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pm_patches_extract_f64", "pm_patches_extract_f32", "pm_patches_accumulate_f64", "pm_patches_finish_f64")
PM_EINVAL, PM_ERANGE = -1, -2

# (L, p, s): stride divides, does not divide, p = L, s > p, s > L, stride 1
AXES = [(10, 4, 3), (10, 4, 4), (10, 4, 1), (7, 7, 2), (12, 3, 5), (9, 2, 20), (5, 1, 1), (37, 4, 3), (40, 4, 3)]


def test_reference_starts():
    assert P.starts(10, 4, 3) == [0, 3, 6]
    assert P.starts(10, 4, 4) == [0, 4, 6]                 # s does not divide L - p: the last start is L - p
    assert P.starts(7, 7, 2) == [0]                        # p = L
    assert P.starts(12, 3, 5) == [0, 5, 9]                 # s > p: gaps closed by the last patch only at the end
    assert P.starts(9, 2, 20) == [0, 7]
    assert P.starts(10, 4, 1) == list(range(7))
    for L, p, s in AXES:
        st = P.starts(L, p, s)
        assert st[0] == 0 and st[-1] == L - p and all(b > a for a, b in zip(st, st[1:]))
        assert all(x % s == 0 for x in st[:-1])


def test_package_grid_rule_is_the_reference():
    from prosper_amd import _lib
    from prosper_amd.utils.patches import patch_starts
    lib = _lib.load()
    for L, p, s in AXES + [(L, p, s) for L in range(1, 14) for p in range(1, L + 1) for s in range(1, 16)]:
        assert patch_starts(L, p, s) == P.starts(L, p, s), (L, p, s)
        assert lib.pm_patches_count(L, p, s) == len(P.starts(L, p, s)), (L, p, s)
    with pytest.raises(ValueError):
        patch_starts(3, 4, 1)
    with pytest.raises(ValueError):
        patch_starts(8, 4, 0)
    assert lib.pm_patches_count(3, 4, 1) == -1 and lib.pm_patches_count(8, 4, 0) == -1


@pytest.mark.parametrize("shape,patch,stride", [((9, 11), (4, 4), 1), ((9, 11), (4, 4), 3), ((13, 7), (3, 5), 2),
                                                ((6, 6), (6, 6), 1), ((3, 10, 9), (4, 3), 3), ((8, 7), (5, 4), 7)])
def test_reference_cover_and_round_trip(shape, patch, stride):
    """Every pixel is covered; average(extract(img)) gives img back within k 2^-52 |pixel|, k the pixel's cover count
    (k - 1 rounded additions and one division)."""
    rng = np.random.RandomState(sum(shape) + stride)
    img = rng.normal(size=shape) * 10.0 ** rng.randint(-3, 4, size=shape)
    cnt = P.cover(shape, patch, stride)
    assert cnt.min() >= 1 and cnt.shape[-2:] == tuple(shape[-2:])
    Y = P.extract(img, patch, stride)
    assert Y.shape == (len(P.grid(shape, patch, stride)), patch[0] * patch[1])
    back = P.average(Y, shape, patch, stride)
    assert back.shape == img.shape
    bound = cnt.reshape(img.shape) * 2.0 ** -52 * np.abs(img)
    assert (np.abs(back - img) <= bound).all(), float((np.abs(back - img) / np.abs(img)).max() / 2.0 ** -52)
    # ... and with the means taken out and handed back
    mu = Y.mean(axis=1)
    back = P.average(Y - mu[:, None], shape, patch, stride, means=mu)
    assert np.abs(back - img).max() <= (cnt.max() + 2) * 2.0 ** -52 * np.abs(img).max()


def test_a_stride_that_leaves_pixels_uncovered_is_refused():
    """The rule covers every pixel when s <= p (or the axis holds at most two patch lengths); a larger stride leaves gaps
    between the regular starts -- the reference's cover count shows them -- and the package refuses it at every layer."""
    from prosper_amd import _lib
    from prosper_amd.utils import patches as U
    assert P.cover((10, 9), (2, 3), 4).min() == 0 and P.cover((8, 8), (2, 2), 5).min() == 0
    assert P.cover((8, 7), (5, 4), 7).min() == 1                     # s > p, L <= 2p: the two patches 0 and L - p meet
    for shape, patch, s in (((10, 9), (2, 3), 4), ((8, 8), 2, 5), ((9, 30), (3, 3), 4)):
        with pytest.raises(ValueError):
            U.extract_patches(np.zeros(shape), patch, stride=s)
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    lib = _lib.load()
    assert lib.pm_patches_finish_f64(p, 9, p, 9, 1, 10, 9, 2, 3, 4, None) == PM_EINVAL
    assert lib.pm_patches_accumulate_f64(p, 6, None, 0, 1, p, 9, 1, 10, 9, 2, 3, 4, None) == PM_EINVAL
    assert lib.pm_patches_extract_f64(p, 9, 1, 10, 9, 2, 3, 4, 0, 1, 0, p, 6, None, None) == PM_EINVAL


def test_dense_grid_cover_count_at_p4():
    cnt = P.cover((12, 12), (4, 4), 1)[0]
    assert cnt.max() == 16 and cnt[0, 0] == 1 and cnt[5, 5] == 16


@pytest.mark.parametrize("kind", ["bsc", "mca"])
def test_reference_denoises_the_bars_image(kind):
    """The bars image's patches are datapoints of the bars model with H = 2p: the exact posterior mean of every patch,
    averaged, is closer to the clean image than the noisy one, and no further than Jensen's inequality allows -- on the
    NumPy reference alone (what the GPU test asserts of the device)."""
    import recon_reference as R
    a, sigma, pi, p, stride = 3.0, 1.0, 0.2, 4, 3
    rng = np.random.RandomState(0)
    clean, noisy, _, _ = P.bars_image(rng, 40, 37, a, pi, sigma, mca=kind == "mca")
    W = P.bars_W(p, a)
    Y, Yc = P.extract(noisy, (p, p), stride), P.extract(clean, (p, p), stride)
    assert np.array_equal(Yc, np.round(Yc / a) * a) and Yc.max() == (a if kind == "mca" else 2 * a)
    if kind == "mca":
        rows = R.enum_mca(Y, np.where(W < 0.05, 0.05, W), 21.0, False, pi, sigma)
    else:
        rows = R.enum_linear(Y, W, sigma, [0., 1.], np.log([1 - pi, pi]))
    out = P.average(rows, noisy.shape, (p, p), stride)
    mse_n, mse_d = ((noisy - clean) ** 2).mean(), ((out - clean) ** 2).mean()
    bound = P.average((rows - Yc) ** 2, noisy.shape, (p, p), stride).mean()
    assert 0.9 < mse_n < 1.1 and mse_d < 0.1 * mse_n and mse_d <= bound * (1 + 1e-12), (mse_n, mse_d, bound)


class _NoDevice(object):
    """A model whose device must not be asked for: argument errors come first."""
    D = 16
    deterministic = False

    @property
    def device(self):
        raise AssertionError("the device was touched before the arguments were checked")

    def reconstruct(self, *a, **k):
        raise AssertionError("reconstruct() was called before the arguments were checked")


def test_argument_errors_come_before_any_device_call(monkeypatch):
    from prosper_amd import _lib
    from prosper_amd.utils import patches as U

    def no_call(*a, **k):
        raise AssertionError("a device entry was called before the arguments were checked")
    monkeypatch.setattr(_lib, "call", no_call)
    monkeypatch.setattr(U, "_device", no_call)
    img = np.zeros((10, 12))
    with pytest.raises(ValueError):
        U.extract_patches(img, 11)                                    # L < p
    with pytest.raises(ValueError):
        U.extract_patches(img, (4, 13))
    with pytest.raises(ValueError):
        U.extract_patches(img, 4, stride=0)
    with pytest.raises(ValueError):
        U.extract_patches(img, (4, 4, 4))
    with pytest.raises(ValueError):
        U.extract_patches(np.zeros((2, 3, 10, 12)), 4)                # colour channels are out of scope
    with pytest.raises(ValueError):
        U.average_patches(np.zeros((5, 16)), (10, 12), 4)             # N does not fit the grid
    with pytest.raises(ValueError):
        U.average_patches(np.zeros((63, 15)), (10, 12), 4)
    with pytest.raises(ValueError):
        U.average_patches(np.zeros((63, 16)), (10, 12), 4, means=np.zeros(62))
    m = _NoDevice()
    with pytest.raises(ValueError):
        U.denoise_image(m, {}, img, patch=(4, 5))                     # p_h p_w != model.D
    with pytest.raises(ValueError):
        U.denoise_image(m, {}, np.zeros((3, 12)))                     # L < p
    with pytest.raises(ValueError):
        U.denoise_image(m, {}, img, chunk=0)
    with pytest.raises(ValueError):
        U.denoise_image(m, {}, img, stride=-1)
    m.D = 15
    with pytest.raises(ValueError):
        U.denoise_image(m, {}, img)                                   # D is not a square and no patch is given


def test_every_model_has_reconstruct_image():
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.mca_et import MCA_ET
    from prosper_amd.em.camodels.mmca_et import MMCA_ET
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    from prosper_amd.em.camodels.tsc_et import TSC_ET
    from prosper_amd.em.camodels.gsc_et import GSC
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.em.mixturemodels.MoP import MoP
    for cls in (BSC_ET, MCA_ET, MMCA_ET, DSC_ET, TSC_ET, GSC, MoG, MoP):
        assert callable(getattr(cls, "reconstruct_image", None)), cls.__name__
        assert "denoise_image" in cls.reconstruct_image.__doc__, cls.__name__


def test_new_entries_in_header_binding_and_both_libraries():
    from prosper_amd import _lib
    header = open(os.path.join(ROOT, "include", "prosper_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    for path in (_lib.LIB_PATH, _lib.LIB_PATH_DET):
        lib = C.CDLL(path)
        for name in NEW + ("pm_patches_count",):
            assert hasattr(lib, name), (path, name)
    assert _lib.load().pm_version() >= 1019 and _lib.MIN_VERSION >= 1019


@pytest.mark.parametrize("det", [False, True])
def test_entries_reject_bad_arguments_without_a_device(det):
    """Every pointer below is host memory (or NULL): a launch would fault, a correct entry returns before one."""
    from prosper_amd import _lib
    lib = _lib.load(det)
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)

    for entry in (lib.pm_patches_extract_f64, lib.pm_patches_extract_f32):
        def ext(img=p, ldi=12, B=1, Hi=10, Wi=12, ph=4, pw=4, s=1, n0=0, n=63, center=0, out=p, ldo=16, means=None):
            return entry(img, ldi, B, Hi, Wi, ph, pw, s, n0, n, center, out, ldo, means, None)
        assert ext(img=None) == PM_EINVAL and ext(out=None) == PM_EINVAL and ext(center=1) == PM_EINVAL
        assert ext(ph=11) == PM_EINVAL and ext(pw=13) == PM_EINVAL and ext(s=0) == PM_EINVAL and ext(ph=0) == PM_EINVAL
        assert ext(B=0) == PM_EINVAL and ext(Hi=0) == PM_EINVAL and ext(ldi=11) == PM_EINVAL and ext(ldo=15) == PM_EINVAL
        assert ext(n0=1, n=63) == PM_EINVAL and ext(n0=-1) == PM_EINVAL and ext(n=-1) == PM_EINVAL     # past the grid: 7 x 9
        assert ext(n=64) == PM_EINVAL and ext(B=2, n=127) == PM_EINVAL
        assert ext(Hi=100, Wi=100, ldi=100, ph=80, pw=80, ldo=6400) == PM_ERANGE                       # D > 4096
        assert ext(Hi=2 ** 30 + 1) == PM_ERANGE
        assert ext(n=0) == 0                                                                           # nothing to do

    def acc(est=p, lde=16, means=None, n0=0, n=63, a=p, lda=12, B=1, Hi=10, Wi=12, ph=4, pw=4, s=1):
        return lib.pm_patches_accumulate_f64(est, lde, means, n0, n, a, lda, B, Hi, Wi, ph, pw, s, None)
    assert acc(est=None) == PM_EINVAL and acc(a=None) == PM_EINVAL
    assert acc(lde=15) == PM_EINVAL and acc(lda=11) == PM_EINVAL and acc(ph=11) == PM_EINVAL and acc(s=0) == PM_EINVAL
    assert acc(n0=60, n=4) == PM_EINVAL and acc(n0=-2) == PM_EINVAL and acc(n=-1) == PM_EINVAL
    assert acc(Wi=2 ** 30 + 1, lda=2 ** 30 + 1) == PM_ERANGE
    assert acc(n=0) == 0

    def fin(a=p, lda=12, out=p, ldo=12, B=1, Hi=10, Wi=12, ph=4, pw=4, s=1):
        return lib.pm_patches_finish_f64(a, lda, out, ldo, B, Hi, Wi, ph, pw, s, None)
    assert fin(a=None) == PM_EINVAL and fin(out=None) == PM_EINVAL
    assert fin(lda=11) == PM_EINVAL and fin(ldo=11) == PM_EINVAL and fin(pw=13) == PM_EINVAL and fin(s=-3) == PM_EINVAL
    assert fin(B=0) == PM_EINVAL and fin(Hi=2 ** 30 + 1) == PM_ERANGE
