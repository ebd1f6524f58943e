"""The weighted overlap average without a GPU: the NumPy statement the GPU tests compare against
(tests/patches_weighted_reference.py) is pinned on tests/patches_reference.py, the two new entries exist in the header, the
binding and both libraries and return their argument errors before they touch a device, and every refusal of the Python
layer is raised before a device is asked for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import patches_reference as P
import patches_weighted_reference as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pm_patches_accumulate_w_f64", "pm_patches_finish_w_f64")
PM_EINVAL, PM_ERANGE = -1, -2

CASES = [((9, 11), (4, 4), 1), ((13, 17), (3, 5), 2), ((8, 7), (5, 4), 7), ((3, 10, 9), (4, 3), 3), ((6, 6), (6, 6), 1)]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _problem(shape, patch, stride):
    rng = np.random.RandomState(sum(shape) + stride)
    N, D = len(P.grid(shape, patch, stride)), patch[0] * patch[1]
    E = rng.normal(size=(N, D)) * 10.0 ** rng.randint(-2, 3, size=(N, 1))
    return N, D, E, rng.normal(size=N) * 3


@pytest.mark.parametrize("shape,patch,stride", CASES)
def test_unit_weights_give_the_plain_sums_and_the_cover_count(shape, patch, stride):
    """All weights 1 (as an explicit weight matrix, as an explicit window, and with neither): num has the bits of the plain
    accumulate of tests/patches_reference.py (1 t = t exactly) and den is the cover count."""
    N, D, E, mu = _problem(shape, patch, stride)
    full = (1,) + tuple(shape) if len(shape) == 2 else tuple(shape)
    cnt = P.cover(shape, patch, stride)
    for means in (None, mu):
        acc = np.zeros(full)                       # the running sum of P.average, before its division
        for k, (b, i, j) in enumerate(P.grid(full, patch, stride)):
            v = E[k].reshape(patch) if means is None else E[k].reshape(patch) + means[k]
            acc[b, i:i + patch[0], j:j + patch[1]] = acc[b, i:i + patch[0], j:j + patch[1]] + v
        assert np.array_equal(_bits((acc / cnt).reshape(shape)), _bits(P.average(E, shape, patch, stride, means=means)))
        for wgt, window in ((np.ones((N, D)), None), (None, np.ones(D)), (None, None), (np.ones((N, D)), np.ones(D))):
            num, den = W.accumulate(np.zeros(full), np.zeros(full), E, shape, patch, stride, wgt=wgt, window=window, means=means)
            assert np.array_equal(_bits(num), _bits(acc))
            assert np.array_equal(den, cnt.astype(np.float64))
            assert np.array_equal(_bits(W.finish(num, den).reshape(shape)), _bits(P.average(E, shape, patch, stride, means=means)))


@pytest.mark.parametrize("shape,patch,stride", CASES)
def test_a_constant_power_of_two_weight_gives_the_plain_average(shape, patch, stride):
    """Scaling by 2^k is exact (no value here comes near the ends of the exponent range), so a constant weight 2^k leaves
    every rounding of the plain average where it was, and (2^k s) / (2^k c) has the bits of s / c."""
    N, D, E, mu = _problem(shape, patch, stride)
    want = P.average(E, shape, patch, stride, means=mu)
    for c in (0.25, 8.0):
        assert np.array_equal(_bits(W.average(E, shape, patch, stride, wgt=np.full((N, D), c), means=mu)), _bits(want))
        assert np.array_equal(_bits(W.average(E, shape, patch, stride, window=np.full(D, c), means=mu)), _bits(want))
        assert np.array_equal(_bits(W.average(E, shape, patch, stride, wgt=np.full((N, D), c), window=np.full(D, 2.0), means=mu)),
                              _bits(want))
    # wmode 1 at V = 0 is the constant weight 1 / floor
    got = W.average(E, shape, patch, stride, wgt=np.zeros((N, D)), wmode=1, floor=0.125, means=mu)
    assert np.array_equal(_bits(got), _bits(want))


def test_reference_weight_rule():
    assert W.weight(None, 0, 0.0, None) == 1.0 and W.weight(3.0, 0, 0.0, None) == 3.0 and W.weight(None, 0, 0.0, 0.5) == 0.5
    assert W.weight(3.0, 0, 0.0, 0.5) == 1.5
    assert W.weight(3.0, 1, 1.0, None) == 0.25 and W.weight(-3.0, 1, 0.5, None) == 2.0 and W.weight(-0.0, 1, 0.5, 4.0) == 8.0
    assert np.isnan(W.weight(np.nan, 1, 1.0, None)) and np.isnan(W.weight(np.nan, 0, 1.0, 2.0))
    # ranges continue from the stored sums: any split gives the bits of one call
    shape, patch, stride = (9, 11), (4, 4), 1
    N, D, E, mu = _problem(shape, patch, stride)
    V = np.random.RandomState(1).uniform(0.0, 2.0, size=(N, D))
    one = W.accumulate(np.zeros((1,) + shape), np.zeros((1,) + shape), E, shape, patch, stride, wgt=V, wmode=1, floor=0.3, means=mu)
    num, den = np.zeros((1,) + shape), np.zeros((1,) + shape)
    for a, b in ((0, 5), (5, 6), (6, N)):
        W.accumulate(num, den, E, shape, patch, stride, wgt=V, wmode=1, floor=0.3, means=mu, n0=a, n=b - a)
    assert np.array_equal(_bits(num), _bits(one[0])) and np.array_equal(_bits(den), _bits(one[1]))
    # 0 / 0 is NaN
    z = W.average(E, shape, patch, stride, wgt=np.zeros((N, D)))
    assert np.isnan(z).all()


def test_new_entries_in_header_binding_and_both_libraries():
    from prosper_amd import _lib
    header = open(os.path.join(ROOT, "include", "prosper_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES[NEW[0]][1]) == 20 and len(_lib.SIGNATURES[NEW[1]][1]) == 9
    for path in (_lib.LIB_PATH, _lib.LIB_PATH_DET):
        lib = C.CDLL(path)
        for name in NEW:
            assert hasattr(lib, name), (path, name)
    assert _lib.load().pm_version() >= 1029 and _lib.MIN_VERSION >= 1029
    assert _lib.load(True).pm_version() >= _lib.MIN_VERSION


@pytest.mark.parametrize("det", [False, True])
def test_entries_reject_bad_arguments_without_a_device(det):
    """Every pointer below is host memory (or NULL): a launch would fault, a correct entry returns before one."""
    from prosper_amd import _lib
    lib = _lib.load(det)
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)

    def acc(est=p, lde=16, wgt=None, ldw=0, wmode=0, floor=0.0, window=None, means=None, n0=0, n=63, num=p, den=p, lda=12,
            B=1, Hi=10, Wi=12, ph=4, pw=4, s=1):
        return lib.pm_patches_accumulate_w_f64(est, lde, wgt, ldw, wmode, floor, window, means, n0, n, num, den, lda, B, Hi, Wi,
                                               ph, pw, s, None)
    assert acc(est=None) == PM_EINVAL and acc(num=None) == PM_EINVAL
    assert acc(wmode=2) == PM_EINVAL and acc(wmode=-1) == PM_EINVAL and acc(wgt=p, ldw=16, wmode=7) == PM_EINVAL
    assert acc(wmode=1, floor=1.0) == PM_EINVAL                                        # variances asked for, none given
    for bad in (-1.0, -1e-300, float("inf"), float("-inf"), float("nan")):
        assert acc(wgt=p, ldw=16, wmode=1, floor=bad, n=0) == PM_EINVAL, bad
    assert acc(wgt=p, ldw=15) == PM_EINVAL and acc(wgt=p, ldw=15, wmode=1, floor=1.0) == PM_EINVAL
    # ... and everything pm_patches_accumulate_f64 refuses, with its codes
    assert acc(lde=15) == PM_EINVAL and acc(lda=11) == PM_EINVAL and acc(ph=11) == PM_EINVAL and acc(s=0) == PM_EINVAL
    assert acc(pw=13) == PM_EINVAL and acc(B=0) == PM_EINVAL and acc(Hi=0) == PM_EINVAL and acc(ph=0) == PM_EINVAL
    assert acc(n0=60, n=4) == PM_EINVAL and acc(n0=-2) == PM_EINVAL and acc(n=-1) == PM_EINVAL and acc(n=64) == PM_EINVAL
    assert acc(Hi=10, Wi=9, lda=9, ph=2, pw=3, s=4, n=1) == PM_EINVAL                  # a stride that leaves pixels uncovered
    assert acc(Wi=2 ** 30 + 1, lda=2 ** 30 + 1) == PM_ERANGE
    assert acc(Hi=100, Wi=100, lda=100, ph=80, pw=80, lde=6400, n=1) == PM_ERANGE      # D > 4096
    assert acc(Hi=100, Wi=100, lda=100, ph=80, pw=80, lde=6400, wgt=p, ldw=6400, wmode=1, floor=1.0, n=1) == PM_ERANGE
    # n == 0 launches nothing, whatever else is given
    assert acc(n=0) == 0 and acc(n=0, den=None) == 0 and acc(n=0, wgt=p, ldw=16, wmode=1, floor=0.0, window=p, means=p) == 0
    assert acc(n0=63, n=0, wgt=p, ldw=20, wmode=0, floor=-5.0) == 0                    # (mode 0 does not read the floor)

    def fin(num=p, den=p, lda=12, out=p, ldo=12, B=1, Hi=10, Wi=12):
        return lib.pm_patches_finish_w_f64(num, den, lda, out, ldo, B, Hi, Wi, None)
    assert fin(num=None) == PM_EINVAL and fin(den=None) == PM_EINVAL and fin(out=None) == PM_EINVAL
    assert fin(lda=11) == PM_EINVAL and fin(ldo=11) == PM_EINVAL
    assert fin(B=0) == PM_EINVAL and fin(Hi=0) == PM_EINVAL and fin(Wi=0) == PM_EINVAL
    assert fin(Hi=2 ** 30 + 1) == PM_ERANGE and fin(Wi=2 ** 30 + 1, lda=2 ** 30 + 1, ldo=2 ** 30 + 1) == PM_ERANGE


class _NoDevice(object):
    """A model whose device must not be asked for: argument errors come first."""
    D = 16
    deterministic = False

    @property
    def device(self):
        raise AssertionError("the device was touched before the arguments were checked")

    def reconstruct(self, *a, **k):
        raise AssertionError("reconstruct() was called before the arguments were checked")

    def _noise_variance(self, model_params):
        return 1.0


def test_python_refusals_come_before_any_device_call(monkeypatch):
    from prosper_amd import _lib
    from prosper_amd.em.mixturemodels.MoP import MoP
    from prosper_amd.utils import patches as U

    def no_call(*a, **k):
        raise AssertionError("a device entry was called before the arguments were checked")
    monkeypatch.setattr(_lib, "call", no_call)
    monkeypatch.setattr(U, "_device", no_call)
    img = np.zeros((10, 12))
    Y = np.zeros((63, 16))
    # average_patches: a window that is not positive and finite, of the wrong shape; weights of the wrong shape
    for bad in (np.zeros(16), -np.ones((4, 4)), np.full(16, np.inf), np.full((4, 4), np.nan), np.ones(15), np.ones((2, 8)),
                np.ones((4, 4, 1))):
        with pytest.raises(ValueError):
            U.average_patches(Y, (10, 12), 4, window=bad)
        with pytest.raises(ValueError):
            U.denoise_image(_NoDevice(), {}, img, window=bad)
        with pytest.raises(ValueError):
            U.denoise_image(_NoDevice(), {}, img, aggregate='precision', floor=1.0, window=bad)
    with pytest.raises(ValueError):
        U.average_patches(Y, (10, 12), 4, weights=np.ones((63, 15)))
    with pytest.raises(ValueError):
        U.average_patches(Y, (10, 12), 4, weights=np.ones((62, 16)))
    m = _NoDevice()
    for bad in ('median', 'Precision', '', None, 1):
        with pytest.raises(ValueError):
            U.denoise_image(m, {}, img, aggregate=bad)
    for bad in (0, 0.0, -1.0, float("inf"), float("nan"), "x", [1.0]):
        with pytest.raises(ValueError):
            U.denoise_image(m, {}, img, aggregate='precision', floor=bad)
    with pytest.raises(NotImplementedError, match="aggregate"):
        U.denoise_image(m, {}, img, aggregate='precision', exact=True)
    with pytest.raises(NotImplementedError, match="aggregate"):
        U.denoise_image(m, {}, img, aggregate='precision', floor=0.5, exact=True)
    # the refusals that exist today come first, in their order
    with pytest.raises(NotImplementedError, match="variance"):
        U.denoise_image(m, {}, img, aggregate='precision', exact=True, variance=True)
    with pytest.raises(ValueError, match="center"):
        U.denoise_image(m, {}, img, aggregate='nonsense', center=True, mask=np.ones_like(img))
    with pytest.raises(ValueError):
        U.denoise_image(m, {}, img, aggregate='precision', chunk=0)
    # MoP has no noise parameter: the default floor cannot be derived
    mop = MoP(16, 3)
    with pytest.raises(ValueError, match="floor"):
        U.denoise_image(mop, {}, img, aggregate='precision')
    with pytest.raises(ValueError, match="floor"):
        mop.reconstruct_image({}, img, aggregate='precision')


def test_noise_variance_hooks():
    from prosper_amd.em.camodels.bsc_et import BSC_ET
    from prosper_amd.em.camodels.dsc_et import DSC_ET
    from prosper_amd.em.camodels.gsc_et import GSC
    from prosper_amd.em.camodels.mca_et import MCA_ET
    from prosper_amd.em.camodels.mmca_et import MMCA_ET
    from prosper_amd.em.camodels.tsc_et import TSC_ET
    from prosper_amd.em.mixturemodels.MoG import MoG
    from prosper_amd.utils import patches as U
    assert U.PRECISION_FLOOR in (1.0, 0.3, 0.1, 0.03, 0.01)
    for cls in (BSC_ET, MCA_ET, MMCA_ET, DSC_ET, TSC_ET):
        assert cls._noise_variance(cls.__new__(cls), {'sigma': np.float64(1.5)}) == 2.25, cls.__name__
    rng = np.random.RandomState(0)
    d = rng.uniform(0.5, 2.0, size=16)
    full = np.diag(d) + 0.01 * (np.ones((16, 16)) - np.eye(16))
    g = GSC.__new__(GSC)
    assert g._noise_variance({'sigma_sq': 0.7}) == 0.7
    assert g._noise_variance({'sigma_sq': d}) == float(np.mean(d))
    assert g._noise_variance({'sigma_sq': full}) == float(np.mean(np.diag(full)))
    m = MoG.__new__(MoG)
    s = rng.uniform(0.5, 2.0, size=(4, 16))
    assert m._noise_variance({'sigmas_sq': s}) == float(np.mean(s))
    sf = np.array([np.diag(row) + 0.01 for row in s])
    assert m._noise_variance({'sigmas_sq': sf}) == float(np.mean(np.array([np.diag(c) for c in sf])))
